// mrts_actions.h -- the action row, stated once for host and device.
//
// One row per (env, cell): the reference's action_plane_space.nvec (vec_env.py:234),
// seven components.  get_action_mask's 78 channels are the components' entries laid
// end to end (component k owns channels ACT_OFF[k] .. ACT_OFF[k] + ACT_LEN[k] - 1);
// getMasks' 79-bit word puts the source bit in front (channel ch = bit ch + 1); the same
// word is the packed mask format (below).
// Users: decode_row (mrts_engine.hip), cell_mask (mrts_rules.h), the stand-in samplers
// (mrts_sampler.hip), the masked action head (mrts_policy.hip).  The oracle keeps
// tables of its own: it is the independent reference.
#ifndef MRTS_ACTIONS_H
#define MRTS_ACTIONS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrts_layout.h"

namespace mrts {

enum { A_NONE = 0, A_MOVE, A_HARVEST, A_RETURN, A_PRODUCE, A_ATTACK };   // UnitAction.TYPE_*: the action-type component's values
enum { ACT_TYPE = 0, ACT_MOVE_DIR, ACT_HARVEST_DIR, ACT_RETURN_DIR, ACT_PRODUCE_DIR, ACT_PRODUCE_TYPE, ACT_ATTACK_CELL,
       ACT_COMPONENTS };
constexpr int ACT_OFF[ACT_COMPONENTS] = {0, 6, 10, 14, 18, 22, 29};
constexpr int ACT_LEN[ACT_COMPONENTS] = {6, 4, 4, 4, 4, 7, 49};

constexpr bool act_offsets_are_running_sums() {
    int sum = 0;
    for (int k = 0; k < ACT_COMPONENTS; k++) {
        if (ACT_OFF[k] != sum) return false;
        sum += ACT_LEN[k];
    }
    return sum == MRTS_MASK_CH;
}
static_assert(act_offsets_are_running_sums(), "ACT_OFF is the running sum of ACT_LEN, MRTS_MASK_CH their total");
static_assert(MRTS_MASK_BITS == MRTS_MASK_CH + 1, "the source bit in front of the channels");
static_assert(ACT_LEN[ACT_TYPE] == A_ATTACK + 1, "one entry per action type");
static_assert(ACT_LEN[ACT_MOVE_DIR] == 4 && ACT_LEN[ACT_HARVEST_DIR] == 4 && ACT_LEN[ACT_RETURN_DIR] == 4 && ACT_LEN[ACT_PRODUCE_DIR] == 4,
              "one entry per direction");
static_assert(ACT_LEN[ACT_PRODUCE_TYPE] == MRTS_NTYPES, "one entry per unit type");
static_assert(ACT_LEN[ACT_ATTACK_CELL] == MRTS_ATTACK_GRID * MRTS_ATTACK_GRID, "one entry per cell of the attack grid");
// decode_row reads the direction of action type ty at r[ty]
static_assert(ACT_MOVE_DIR == A_MOVE && ACT_HARVEST_DIR == A_HARVEST && ACT_RETURN_DIR == A_RETURN, "direction component = action type");

// Component k's offset and length for a k known only at run time, from packed bytes:
// a shift and a mask instead of a table in memory (k >= ACT_COMPONENTS: 0, 0).
constexpr uint64_t act_pack(const int (&t)[ACT_COMPONENTS]) {
    uint64_t w = 0;
    for (int k = 0; k < ACT_COMPONENTS; k++) w |= (uint64_t)t[k] << (8 * k);
    return w;
}
static_assert(ACT_COMPONENTS <= 8 && MRTS_MASK_CH < 256, "a byte per component in one 64-bit word");
constexpr uint64_t ACT_OFF_BYTES = act_pack(ACT_OFF), ACT_LEN_BYTES = act_pack(ACT_LEN);
__host__ __device__ inline int comp_off(int k) { return (int)((ACT_OFF_BYTES >> (8 * k)) & 0xFF); }
__host__ __device__ inline int comp_len(int k) { return (int)((ACT_LEN_BYTES >> (8 * k)) & 0xFF); }
// the component that owns channel ch
__host__ __device__ inline int comp_of(int ch) {
    int k = 0;
    for (int j = 1; j < ACT_COMPONENTS; j++) k += ch >= ACT_OFF[j];
    return k;
}
// a component's valid entries as bits 0 .. len - 1, from a row's 78 channels as bits lo (0..63) | hi (64..77)
__host__ __device__ inline uint64_t comp_bits(uint64_t lo, uint64_t hi, int off, int len) {
    return ((lo >> off) | (off ? (hi << (64 - off)) : 0ull)) & ((1ull << len) - 1ull);
}
// Packed masks: getMasks' 79-bit word of a row as it is, three uint32 bit patterns per
// row, packed [N][HW][MASK_PACKED_WORDS] int32 (include/microrts_amd.h states the same):
//   word j, bit b = bit 32 j + b of the 79-bit word; bit 0 = the source channel,
//   bit ch + 1 = mask channel ch; bits 79..95 are zero in everything the library writes
//   and ignored by everything that reads.  A row is 12 bytes: 4-byte alignment only.
constexpr int MASK_PACKED_WORDS = 3;
static_assert(MRTS_MASK_BITS > 64 && MRTS_MASK_BITS <= 32 * MASK_PACKED_WORDS, "a row's bits fill the third word partly");
constexpr uint32_t MASK_PACKED_W2 = (1u << (MRTS_MASK_BITS - 64)) - 1u;   // the third word's bits that belong to the row
// a packed row's channels as comp_bits takes them: lo = channels 0..63, hi = channels 64..77 (bits 79..95 dropped)
__host__ __device__ inline uint64_t packed_lo(uint32_t w0, uint32_t w1, uint32_t w2) {
    return (uint64_t)(w0 >> 1) | ((uint64_t)w1 << 31) | ((uint64_t)(w2 & 1u) << 63);
}
__host__ __device__ inline uint64_t packed_hi(uint32_t w2) { return (uint64_t)((w2 & MASK_PACKED_W2) >> 1); }
// A uniform pick among n entries from one random word.  With n = the component's length it
// is the no-valid-entry draw: what every sampler writes for a component the mask leaves empty.
__host__ __device__ inline int draw_uniform(uint32_t r, int n) { return (int)(((uint64_t)r * (uint32_t)n) >> 32); }

// Packed actions: a row's seven components in one uint32 bit pattern, packed [N][HW] int32
// (include/microrts_amd.h states the same):
//   component k's value in ACT_WBITS[k] bits from bit ACT_WOFF[k] -- the fewest bits that hold
//   0 .. ACT_LEN[k] - 1, the fields laid end to end from bit 0 --
//   bit ACT_WFLAG + k = component k's INVALID flag; the bits above are zero in everything the
//   library writes and ignored by everything that reads.
// A word stands for the dense row act_word_get gives: component k is -1 when flag k is set and
// the field's value otherwise (a field value >= ACT_LEN[k] is out of range as the same int64 is).
// act_word_pack puts component k into its field when it lies in [0, 2^ACT_WBITS[k]); otherwise
// the field is 0 and the flag is set: such a component is out of range in the dense row as well,
// so every reader treats pack(row) as it treats the row.
constexpr int act_field_bits(int len) {
    int b = 0;
    while ((1 << b) < len) b++;
    return b;
}
constexpr int ACT_WBITS[ACT_COMPONENTS] = {act_field_bits(ACT_LEN[0]), act_field_bits(ACT_LEN[1]), act_field_bits(ACT_LEN[2]),
                                           act_field_bits(ACT_LEN[3]), act_field_bits(ACT_LEN[4]), act_field_bits(ACT_LEN[5]),
                                           act_field_bits(ACT_LEN[6])};
constexpr int act_field_off(int k) {
    int o = 0;
    for (int j = 0; j < k; j++) o += ACT_WBITS[j];
    return o;
}
constexpr int ACT_WOFF[ACT_COMPONENTS] = {act_field_off(0), act_field_off(1), act_field_off(2), act_field_off(3),
                                          act_field_off(4), act_field_off(5), act_field_off(6)};
constexpr int ACT_WFLAG = act_field_off(ACT_COMPONENTS);   // the first flag bit: the fields' total width
constexpr int ACT_WUSED = ACT_WFLAG + ACT_COMPONENTS;       // bits that carry anything
static_assert(ACT_COMPONENTS == 7, "ACT_WBITS / ACT_WOFF list seven components");
static_assert(ACT_WFLAG == 20 && ACT_WUSED == 27 && ACT_WUSED <= 32, "20 field bits + 7 flags in one 32-bit word");
static_assert(ACT_WOFF[ACT_ATTACK_CELL] == 14 && ACT_WBITS[ACT_ATTACK_CELL] == 6 && ACT_WBITS[ACT_TYPE] == 3, "the documented layout");
constexpr uint64_t ACT_WOFF_BYTES = act_pack(ACT_WOFF), ACT_WBITS_BYTES = act_pack(ACT_WBITS);
__host__ __device__ inline int act_word_off(int k) { return (int)((ACT_WOFF_BYTES >> (8 * k)) & 0xFF); }
__host__ __device__ inline int act_word_bits(int k) { return (int)((ACT_WBITS_BYTES >> (8 * k)) & 0xFF); }
// component k (< ACT_COMPONENTS) of the dense row the word stands for
__host__ __device__ inline int act_word_get(uint32_t w, int k) {
    return ((w >> (ACT_WFLAG + k)) & 1u) ? -1 : (int)((w >> act_word_off(k)) & ((1u << act_word_bits(k)) - 1u));
}
__host__ __device__ inline uint32_t act_word_put(uint32_t w, int k, long long v) {
    return (v >= 0 && v < (1ll << act_word_bits(k))) ? w | ((uint32_t)v << act_word_off(k)) : w | (1u << (ACT_WFLAG + k));
}
__host__ __device__ inline uint32_t act_word_pack(const int64_t* row) {
    uint32_t w = 0;
    for (int k = 0; k < ACT_COMPONENTS; k++) w = act_word_put(w, k, row[k]);
    return w;
}

}  // namespace mrts
#endif
