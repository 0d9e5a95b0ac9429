"""Dump the step / bot / fused LDS layout figures of a built libmicrorts_amd.so (CPU only: the
library loads without a GPU), one line per map size, for w in 1..48 and h in 1..64:

    w h | own NT unfused, fused | unfused bytes | bot bytes | fused bytes, fused + fog | early |
    bytes at NT 64, 128, 256 for (unfused, fused) x (full, fog)

    python dump_layout.py path/to/libmicrorts_amd.so > dump.txt ; sha256sum dump.txt

Works on both sides of the change that made the layout single-source: a library with
mrts_engine_step_layout is asked through it, an older one through the six queries it replaced.
"""
import ctypes
import sys


class StepLayout(ctypes.Structure):
    _fields_ = [("NT", ctypes.c_int), ("early", ctypes.c_int), ("lds_bytes", ctypes.c_size_t)]


def queries(lib):
    """-> nt(hw, fused), bytes(hw, w, fused, partial, NT), early(hw, w), bot(hw, w)"""
    i, z = ctypes.c_int, ctypes.c_size_t
    bot = lib.mrts_engine_bot_lds_bytes
    bot.restype, bot.argtypes = z, [i, i]
    if hasattr(lib, "mrts_engine_step_layout"):
        q = lib.mrts_engine_step_layout
        q.restype, q.argtypes = StepLayout, [i] * 5
        # the old library's NT took no width and no fog: any does
        return (lambda hw, fused: q(hw, 1, fused, 0, 0).NT, lambda hw, w, fused, partial, nt: q(hw, w, fused, partial, nt).lds_bytes,
                lambda hw, w: q(hw, w, 1, 0, 0).early, bot)
    nt, grp, early = lib.mrts_engine_step_nt, lib.mrts_engine_group_lds_bytes, lib.mrts_engine_early_bot_ok
    unf, fus = lib.mrts_engine_lds_bytes, lib.mrts_engine_fused_lds_bytes
    nt.restype, nt.argtypes = i, [i, i]
    grp.restype, grp.argtypes = z, [i] * 5
    early.restype, early.argtypes = i, [i, i]
    unf.restype, unf.argtypes = z, [i, i]
    fus.restype, fus.argtypes = z, [i, i, i]

    def nbytes(hw, w, fused, partial, NT):
        if NT:
            return grp(hw, w, fused, NT, partial)
        return fus(hw, w, partial) if fused else unf(hw, w)

    return nt, nbytes, early, bot


def main(path):
    nt, nbytes, early, bot = queries(ctypes.CDLL(path))
    for w in range(1, 49):
        for h in range(1, 65):
            hw = w * h
            row = [w, h, nt(hw, 0), nt(hw, 1), nbytes(hw, w, 0, 0, 0), bot(hw, w), nbytes(hw, w, 1, 0, 0), nbytes(hw, w, 1, 1, 0),
                   early(hw, w)]
            row += [nbytes(hw, w, fused, partial, NT) for NT in (64, 128, 256) for fused in (0, 1) for partial in (0, 1)]
            print(*row)


if __name__ == "__main__":
    main(sys.argv[1])
