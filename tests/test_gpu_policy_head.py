"""The masked action head on the MI355X (gym_microrts.policy_head over
csrc/mrts_policy.hip) against the float64 reference, the Philox helper and the input
sets of test_policy_head.py: sampled actions, determinism and sharding, sample ==
evaluate, accuracy against a float32 torch Categorical, the backward against float64
autograd, invalid actions, and a rollout plus one driver update end to end.

Measured on the MI355X (profiles/policy_head/accuracy.json holds every case): the
fused log-prob / entropy are within 1.3 float32 ulps of the float64 sums on every input
set; the gradients' largest error is 4.7 ulps of max|g| (16x16_sparse, 1.12e-6 against
the torch path's 1.02e-6), 3.7 ulps or less elsewhere."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import REPO
from test_policy_head import CH, INPUT_IDS, LEN, LP_INVALID, OFF, Reference, inputs, no_valid_draw

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ACCURACY_JSON = os.path.join(REPO, "profiles", "policy_head", "accuracy.json")
_dev = {}


def _torch():
    import torch

    return torch


def dev_inputs(name):
    """The input set as device tensors (built once): logits [n*hw, 78] f32, mask, source i32."""
    if name not in _dev:
        torch = _torch()
        d = inputs(name)
        _dev[name] = (torch.from_numpy(d["logits"]).cuda(), torch.from_numpy(d["mask"]).cuda(), torch.from_numpy(d["source"]).cuda())
    return _dev[name]


def fused_sample(name, env0=0, rows=slice(None)):
    from gym_microrts import policy_head

    d = inputs(name)
    lg, m, s = dev_inputs(name)
    lg = lg.reshape(d["n"], d["hw"], CH)
    return policy_head.sample(lg[rows].contiguous(), m[rows].contiguous(), s[rows].contiguous(), seed=d["seed"], step=d["step"], env0=env0)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def record(section, name, **figures):
    """Merge one case's measured errors into profiles/policy_head/accuracy.json (a
    read-only checkout keeps the committed file; the figures are printed either way)."""
    try:
        with open(ACCURACY_JSON) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc.setdefault(section, {})[name] = {k: float(v) for k, v in figures.items()}
    try:
        os.makedirs(os.path.dirname(ACCURACY_JSON), exist_ok=True)
        with open(ACCURACY_JSON, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def torch_head(lg, mask, src, actions):
    """The reference's head in float32 torch: Categorical over where(mask, logits, -1e8)
    per component (experiments/ppo_gridnet.py:164-167, 228-247); per env the components'
    float32 values summed in float64 and rounded once.  Returns float32 (logprob, entropy),
    differentiable in lg."""
    torch = _torch()
    from torch.distributions import Categorical

    n, hw = src.shape
    valid = (mask.reshape(n * hw, CH) != 0) & (src.reshape(-1, 1) != 0)
    a = actions.reshape(n * hw, 7)
    lp, ent = 0, 0
    for k, (off, ln) in enumerate(zip(OFF, LEN)):
        cat = Categorical(logits=torch.where(valid[:, off:off + ln], lg[:, off:off + ln], torch.tensor(-1e8, device=lg.device)))
        lp = lp + cat.log_prob(a[:, k]).double()
        ent = ent + cat.entropy().double()
    return lp.reshape(n, hw).sum(1).float(), ent.reshape(n, hw).sum(1).float()


# ------------------------------------------------------------------ 1. sampled actions
@pytest.mark.parametrize("name", INPUT_IDS)
def test_sampled_actions_equal_the_inverse_cdf_reference(name):
    d = inputs(name)
    a, _, _ = fused_sample(name)
    a = a.cpu().numpy()
    assert a.shape == (d["n"], d["hw"], 7) and a.dtype == np.int64
    diff = (a != d["actions"]) & d["keep"]
    assert not diff.any(), f"{int(diff.sum())} components differ, first at {np.argwhere(diff)[:5].tolist()}"
    srcrow = d["source"] != 0
    for k, c in enumerate(d["ref"].comp):   # every component with valid entries is valid under the mask
        ak = a[:, :, k]
        assert ((ak >= 0) & (ak < LEN[k])).all()
        assert np.take_along_axis(c["v"], ak[..., None], -1)[..., 0][c["some"]].all(), f"component {k}"
    np.testing.assert_array_equal(a[~srcrow], no_valid_draw(d["r"]).astype(np.int64)[~srcrow])


# ------------------------------------------------------------------ 2. determinism, sharding
@pytest.mark.parametrize("name", ["9x13_sparse", "16x16_sparse", "24x24_sparse"])
def test_two_calls_give_equal_bits_and_a_shard_equals_its_slice(name):
    torch = _torch()
    def bits(x):
        return x if x.dtype == torch.int64 else x.view(torch.int32)

    one, two = fused_sample(name), fused_sample(name)
    for x, y in zip(one, two):
        assert torch.equal(bits(x), bits(y))
    shard = fused_sample(name, env0=20, rows=slice(20, None))
    for x, y in zip(one, shard):
        assert torch.equal(bits(x[20:]), bits(y))
    np.testing.assert_array_equal(shard[0].cpu().numpy()[inputs(name)["keep"][20:]],
                                  inputs(name)["actions"][20:][inputs(name)["keep"][20:]])


# ------------------------------------------------------------------ 3. sample == evaluate
@pytest.mark.parametrize("name", INPUT_IDS)
def test_sample_and_evaluate_agree_bit_for_bit(name):
    torch = _torch()
    from gym_microrts import policy_head

    d = inputs(name)
    lg, m, s = dev_inputs(name)
    a, lp, ent = fused_sample(name)
    lp2, ent2 = policy_head.evaluate(lg, m, s, a)
    assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(ent.view(torch.int32), ent2.view(torch.int32))
    # the rollout buffer's forms: [N, HW, 78] logits, float copies of mask / source, flat actions
    lp3, ent3 = policy_head.evaluate(lg.reshape(d["n"], d["hw"], CH), m.float(), s.float(), a.reshape(d["n"], -1))
    assert torch.equal(lp.view(torch.int32), lp3.view(torch.int32)) and torch.equal(ent.view(torch.int32), ent3.view(torch.int32))


# ------------------------------------------------------------------ 4. accuracy
@pytest.mark.parametrize("name", INPUT_IDS)
def test_logprob_and_entropy_accuracy_against_float64(name):
    """|fused - float64| <= max(2 * max|torch float32 - float64|, 2 float32 ulps of the result), per env."""
    d = inputs(name)
    lg, m, s = dev_inputs(name)
    a, lp, ent = fused_sample(name)
    an = a.cpu().numpy()
    want_lp, want_ent = d["ref"].logprob(an), d["ref"].entropy()
    tlp, tent = torch_head(lg, m, s, a)
    figures = {}
    for what, got, tor, want in (("logprob", lp, tlp, want_lp), ("entropy", ent, tent, want_ent)):
        err_f = np.abs(got.cpu().numpy().astype(np.float64) - want)
        err_t = np.abs(tor.detach().cpu().numpy().astype(np.float64) - want)
        figures[f"{what}_fused_max_err"] = err_f.max()
        figures[f"{what}_torch_max_err"] = err_t.max()
        figures[f"{what}_fused_max_err_ulps"] = (err_f / ulp32(want)).max()
        figures[f"{what}_max_abs"] = np.abs(want).max()
    print(name, figures)
    record("forward", name, **figures)
    for what, got, tor, want in (("logprob", lp, tlp, want_lp), ("entropy", ent, tent, want_ent)):
        err_f = np.abs(got.cpu().numpy().astype(np.float64) - want)
        bound = np.maximum(2.0 * figures[f"{what}_torch_max_err"], 2.0 * ulp32(want))
        assert (err_f <= bound).all(), (what, figures)


# ------------------------------------------------------------------ 5. backward
def reference_gradient(d, actions, g_lp, g_ent):
    """float64 autograd of the reference head (torch, CPU): d(sum_e g_lp[e] logprob[e] + g_ent[e] entropy[e]) / d logits."""
    torch = _torch()
    n, hw = d["n"], d["hw"]
    l = torch.from_numpy(d["logits"]).double().requires_grad_(True)
    valid = torch.from_numpy(d["ref"].valid.reshape(n * hw, CH))
    a = torch.from_numpy(actions.reshape(n * hw, 7))
    w_lp = torch.from_numpy(np.repeat(g_lp.astype(np.float64), hw))
    w_ent = torch.from_numpy(np.repeat(g_ent.astype(np.float64), hw))
    loss = 0
    for k, (off, ln) in enumerate(zip(OFF, LEN)):
        v = valid[:, off:off + ln]
        some = v.any(-1)
        veff = v | ~some[:, None]   # a component without valid entries: any finite softmax, its weight is 0
        logp = torch.log_softmax(l[:, off:off + ln].masked_fill(~veff, -float("inf")), -1)
        safe = torch.where(veff, logp, torch.zeros_like(logp))
        H = -(safe.exp() * veff * safe).sum(-1)
        picked = torch.gather(safe, 1, a[:, k:k + 1])[:, 0]
        ok = torch.gather(v, 1, a[:, k:k + 1])[:, 0]
        lp = torch.where(ok, picked, torch.full_like(picked, LP_INVALID))
        loss = loss + ((w_lp * lp + w_ent * H) * some).sum()
    loss.backward()
    return l.grad.numpy()


@pytest.mark.parametrize("name", INPUT_IDS)
def test_backward_against_float64_autograd(name):
    """Elementwise |fused - float64| <= max(2 * max|torch float32 - float64|, 4 float32 ulps of max|g|);
    masked entries and non-source rows are +0.0f as bits; a NaN-filled buffer comes back finite."""
    torch = _torch()
    from gym_microrts import _native, policy_head

    d = inputs(name)
    n, hw = d["n"], d["hw"]
    lg, m, s = dev_inputs(name)
    a, _, _ = fused_sample(name)
    rng = np.random.default_rng(d["seed"] + 1000)
    g_lp, g_ent = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    glp_d, gent_d = torch.from_numpy(g_lp).cuda(), torch.from_numpy(g_ent).cuda()
    want = reference_gradient(d, a.cpu().numpy(), g_lp, g_ent)

    x = lg.clone().requires_grad_(True)
    lp, ent = policy_head.evaluate(x, m, s, a)
    (lp * glp_d + ent * gent_d).sum().backward()
    got = x.grad
    assert got.shape == lg.shape and got.dtype == torch.float32

    raw = torch.full((n * hw, CH), float("nan"), device="cuda")   # the kernel writes every element
    _native.check(_native.lib().mrts_policy_evaluate_backward(torch.cuda.current_stream().cuda_stream, lg.data_ptr(), m.data_ptr(),
                                                              s.data_ptr(), n, hw, a.data_ptr(), glp_d.data_ptr(), gent_d.data_ptr(),
                                                              raw.data_ptr()))
    assert bool(torch.isfinite(raw).all())
    assert torch.equal(raw.view(torch.int32), got.view(torch.int32))
    masked = torch.from_numpy(~d["ref"].valid.reshape(n * hw, CH)).cuda()
    assert bool((got.view(torch.int32)[masked] == 0).all())   # +0.0f, not -0.0f

    y = lg.clone().requires_grad_(True)
    tlp, tent = torch_head(y, m, s, a)
    (tlp * glp_d + tent * gent_d).sum().backward()
    err_f = np.abs(got.cpu().numpy().astype(np.float64) - want)
    err_t = np.abs(y.grad.cpu().numpy().astype(np.float64) - want)
    gmax = np.abs(want).max()
    figures = dict(fused_max_err=err_f.max(), torch_max_err=err_t.max(), max_abs_grad=gmax,
                   fused_max_err_ulps_of_max=err_f.max() / ulp32(gmax) if gmax else 0.0)
    print(name, figures)
    record("backward", name, **figures)
    assert (err_f <= max(2.0 * err_t.max(), 4.0 * float(ulp32(gmax)))).all(), figures


# ------------------------------------------------------------------ 6. invalid actions
def test_invalid_actions_give_minus_1e8_and_no_fault():
    """One env, 9x13, every cell a source cell with components 1 and 6 partly valid: a
    masked entry of component 1 at cell 3 and an out-of-range index of component 6 at
    cell 7 (negative and huge at cells 9 and 11) each contribute exactly -1e8; the
    reference alone says so, and the backward drops their indicator term."""
    torch = _torch()
    from gym_microrts import policy_head

    hw = 117
    rng = np.random.default_rng(5)
    mask = np.zeros((1, hw, CH), np.int32)
    mask[0, :, 0] = 1
    mask[0, :, [6, 8]] = 1
    mask[0, :, 29:40] = 1
    src = np.ones((1, hw), np.int32)
    lg = rng.standard_normal((hw, CH)).astype(np.float32)
    a = np.zeros((1, hw, 7), np.int64)
    a[0, :, 1] = 2
    a[0, :, 6] = 5
    ref = Reference(lg, mask, src)
    clean = ref.logprob(a)[0]
    a[0, 3, 1] = 1                 # masked
    a[0, 7, 6] = 49                # one past the component
    a[0, 9, 6] = -1
    a[0, 11, 6] = 2 ** 40
    a[0, 13, 2] = 77               # a component without valid entries ignores its action
    want = ref.logprob(a)[0]
    assert -4.0e8 - 1e3 < want < -4.0e8 + 1e3 and abs(clean) < 1e3
    x = torch.from_numpy(lg).cuda().requires_grad_(True)
    lp, ent = policy_head.evaluate(x, torch.from_numpy(mask).cuda(), torch.from_numpy(src).cuda(), torch.from_numpy(a).cuda())
    assert abs(float(lp[0].detach()) - want) <= 2 * float(ulp32(want))
    assert abs(float(ent[0].detach()) - ref.entropy()[0]) <= 2 * float(ulp32(ref.entropy()[0]))
    lp.sum().backward()
    g = x.grad.cpu().numpy()
    assert np.isfinite(g).all()
    np.testing.assert_allclose(g[7, 29:40], -ref.comp[6]["p"][0, 7, :11], rtol=1e-5, atol=1e-7)   # no indicator term
    np.testing.assert_allclose(g[3, [6, 8]], -ref.comp[1]["p"][0, 3, [0, 2]], rtol=1e-5, atol=1e-7)
    assert (g[13, 10:14] == 0).all()


# ------------------------------------------------------------------ 7. end to end
def _driver():
    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rollout_driven_by_the_fused_head():
    """50 steps of 16 selfplay envs (16x16) under a seeded GridNet: every sampled component
    with valid entries is valid on every source cell, and the engine raises no error flag."""
    torch = _torch()
    from gym_microrts import policy_head
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    drv = _driver()
    env = MicroRTSGridModeVecEnv(num_selfplay_envs=16, num_bot_envs=0, max_steps=2000, map_paths=["maps/16x16/basesWorkers16x16.xml"],
                                 reward_weight=np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0]), device="cuda:0", return_tensors=True)
    torch.manual_seed(7)
    h, w, planes = env.observation_space.shape
    net = drv.GridNet(planes, h, w).cuda()
    obs = env.reset()
    acted = 0
    for t in range(50):
        mask, src = env.get_action_mask(), env.source_unit_mask
        with torch.no_grad():
            logits, _ = net(obs.float())
        a, lp, ent = policy_head.sample(logits, mask, src, seed=3, step=t)
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(ent).all()) and bool((ent >= 0).all())
        rows = src.bool()
        for k, (off, ln) in enumerate(zip(OFF, LEN)):
            mk = mask[:, :, off:off + ln]
            picked = torch.gather(mk, 2, a[:, :, k:k + 1])[:, :, 0]
            some = mk.any(-1) & rows
            assert bool((picked[some] == 1).all()), f"component {k} picked an invalid entry at step {t}"
        acted += int(rows.sum())
        obs, _, _, _ = env.step(a)
    assert acted > 50, acted   # units did act
    assert env.error_flags() == 0
    env.close()


def test_driver_update_with_the_fused_head_and_its_logprobs_against_the_torch_head():
    """One update of examples/ppo_gridnet_driver.py with head="fused" gives finite losses;
    the first rollout's per-sample log-probs equal the torch head's on the same
    observations, masks and actions once the torch side's sum of -log(len_k) over the
    components without valid entries is taken out (check 4's tolerance, against the
    float64 reference on the same logits)."""
    torch = _torch()
    drv = _driver()
    stats = drv.run(num_selfplay_envs=16, num_steps=8, updates=1, api="tensor", head="fused", keep_first_rollout=True, log=lambda s: None)
    assert stats["finite"] and stats["engine_error_flags"] == 0 and stats["head"] == "fused"
    fr = stats["first_rollout"]
    T, n, hw = fr["source"].shape
    h = w = int(round(hw ** 0.5))
    net = drv.GridNet(fr["obs"].shape[-1], h, w).cuda()
    net.load_state_dict(fr["state_dict"])
    obs, mask, src, act = (fr[k].reshape((T * n,) + fr[k].shape[2:]) for k in ("obs", "mask", "source", "actions"))
    with torch.no_grad():
        logits, _ = net(obs)
        _, tlp, _, _ = drv.policy(net, obs, mask.float(), hw, action=act)
    ref = Reference(logits.cpu().numpy(), mask.cpu().numpy(), src.cpu().numpy())
    want = ref.logprob(act.cpu().numpy())
    const = sum((~c["some"]).sum(1) * np.log(float(LEN[k])) for k, c in enumerate(ref.comp))   # the torch head's -log(len) terms
    err_t = np.abs(tlp.cpu().numpy().astype(np.float64) + const - want)
    err_f = np.abs(fr["logprob"].reshape(-1).cpu().numpy().astype(np.float64) - want)
    print("driver logprob: fused max err", err_f.max(), "torch max err", err_t.max())
    assert (err_f <= np.maximum(2.0 * err_t.max(), 2.0 * ulp32(want))).all()
