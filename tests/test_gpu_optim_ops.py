"""The AdamW and loss-scale kernels (csrc/optim.hip) on flat buffers, entry point by entry point: pssr_adamw_step,
pssr_adamw_step_dev, pssr_adamw_step_amp, pssr_amp_check.

Every step is compared with the float64 recurrence of tests/_optim_ref64.py started from the f32 state the kernel itself left, so
the bound is that of ONE f32 step.  The bound (docstring of _optim_ref64): per element, MARGIN = 2 times
    m: 5 roundings  (g gs, 1 - b1, two products, the sum)                                  x 2^-24 x (|b1 m| + |(1 - b1) g gs|)
    v: 7 roundings  (g gs twice, 1 - b2, three products, the sum)                          x 2^-24 x (b2 v + (1 - b2) (g gs)^2)
    p: 20 roundings (3 decay, 5 m, 8 denominator, 4 quotient / step size / product / sum)  x 2^-24 x (|p (1 - lr wd)| + |update terms|)
       + |update terms| x (3 x 2^-24 / (1 - b1^t) + 1.5 x 2^-24 / (1 - b2^t))              the bias corrections' own term
plus 2^-126 per quantity for underflow.  tests/test_optim_ref64.py shows on these inputs that torch.optim.AdamW in f32 stays inside
(worst error / bound 0.05 for p, 0.16 for m, 0.14 for v) and that six wrong recurrences leave it.  Each test prints the worst
error / bound it saw."""
import struct

import numpy as np
import pytest
import torch

import _optim_ref64 as R

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 3, 4, 5, 7, 1023, 1027)
BIG = 4 * 256 * 4096 + 5            # the 4096 workgroups of adamw_kernel make a second trip, and a tail is left
ENTRIES = ("step", "dev", "amp")
AMP_SCALE = 1024.0


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _dev_state(step, lr):
    """int64[2]: the step count so far and, in the next word, the f32 bits of lr"""
    return torch.tensor([step, _bits(lr)], dtype=torch.int64, device="cuda")


def _amp_state(scale=AMP_SCALE, good=0, skipped=0, flag=0):
    return torch.tensor([_bits(scale), good, skipped, flag], dtype=torch.int32, device="cuda")


def _call(entry, p, g, m, v, h, step, *, state=None, amp=None, policy=(2.0, 0.5, 1000)):
    """one step through an entry point; `step` is the 1-based count of this step.  The amp entry gets gradients that the caller
    scaled by the loss scale (a power of two: exact)."""
    from pssr2_amd import ops
    if entry == "step":
        ops.adamw_step(p, g, m, v, h.lr, h.beta1, h.beta2, h.eps, h.wd, step, h.grad_scale)
    elif entry == "dev":
        ops.adamw_step_dev(p, g, m, v, state, h.beta1, h.beta2, h.eps, h.wd, h.grad_scale)
    else:
        ops.adamw_step_amp(p, g, m, v, state, h.beta1, h.beta2, h.eps, h.wd, amp, policy[0], policy[1], policy[2], h.grad_scale)


def _offset_view(t, off):
    """the values of t in a view at element offset `off` of a larger buffer"""
    buf = torch.zeros(t.numel() + off + 3, dtype=t.dtype, device="cuda")
    view = buf[off:off + t.numel()]
    view.copy_(t)
    return view


def _three_steps(entry, name, n, offset=0):
    """three steps of a configuration, each checked against float64; returns the worst error / bound of (p, m, v)"""
    cfg = R.CONFIGS[name]
    h = cfg.h
    p0, gs, m0, v0 = R.inputs(name, n)
    p, m, v = (_offset_view(t, offset) for t in (p0, m0, v0))
    state = _dev_state(cfg.step0 - 1, h.lr) if entry != "step" else None
    amp = _amp_state() if entry == "amp" else None
    worst = [0.0, 0.0, 0.0]
    for k, g_host in enumerate(gs):
        step = cfg.step0 + k
        before = [t.double().cpu() for t in (p, m, v)]
        g64 = g_host.double()
        g = _offset_view(g_host * AMP_SCALE if entry == "amp" else g_host, offset)
        if entry == "amp":
            assert bool(torch.isfinite(g).all())
        _call(entry, p, g, m, v, h, step, state=state, amp=amp)
        args = (before[0], g64, before[1], before[2])
        want = R.adamw64(*args, h, step)
        bound = R.adamw_bound(*args, h, step)
        r = R.ratios([t.cpu() for t in (p, m, v)], want, bound)
        assert max(r) <= 1.0, f"{entry} {name} n={n} offset={offset} step {step}: error / bound (p, m, v) = {r}"
        worst = [max(a, b) for a, b in zip(worst, r)]
        if state is not None:
            assert int(state[0]) == step
    return worst


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_adamw_small_sizes_against_f64(entry, name):
    """body only (4), tail only (1, 2, 3), both (5, 7, 1023, 1027), three steps each"""
    worst = [0.0, 0.0, 0.0]
    for n in SMALL:
        worst = [max(a, b) for a, b in zip(worst, _three_steps(entry, name, n))]
    print(f"adamw {entry} {name}: worst error / bound (p, m, v) = {worst[0]:.4f} {worst[1]:.4f} {worst[2]:.4f}")


@pytest.mark.parametrize("n", [1, 2, 3])
def test_adamw_step_takes_a_misaligned_view_below_four_elements(n):
    """n < 4 has no float4 body: every entry point allows a view at element offset 1"""
    for entry in ENTRIES:
        r = _three_steps(entry, "base", n, offset=1)
        print(f"adamw {entry} base n={n} offset 1: worst error / bound (p, m, v) = {r}")


@pytest.mark.parametrize("entry", ENTRIES)
def test_adamw_second_grid_trip_against_f64(entry):
    worst = _three_steps(entry, "base", BIG)
    print(f"adamw {entry} base n={BIG}: worst error / bound (p, m, v) = {worst[0]:.4f} {worst[1]:.4f} {worst[2]:.4f}")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["base", "late", "g_tiny", "g_big_scaled"])
def test_adamw_body_and_tail_store_the_same_bits(entry, name):
    """the float4 body and the scalar tail are two copies of the update: the same (p, g, m, v) at elements 4..6 of an n = 7 buffer (tail)
    and of an n = 8 buffer (body) must give identical bits"""
    cfg = R.CONFIGS[name]
    p0, gs, m0, v0 = R.inputs(name, 8)
    out = {}
    for n in (7, 8):
        p, m, v = (t[:n].clone().cuda() for t in (p0, m0, v0))
        state = _dev_state(cfg.step0 - 1, cfg.h.lr) if entry != "step" else None
        amp = _amp_state() if entry == "amp" else None
        for k in range(R.STEPS):
            g = (gs[k][:n] * (AMP_SCALE if entry == "amp" else 1.0)).cuda()
            _call(entry, p, g, m, v, cfg.h, cfg.step0 + k, state=state, amp=amp)
        out[n] = [t.cpu().view(torch.int32) for t in (p, m, v)]
    for what, tail, body in zip("pmv", out[7], out[8]):
        assert torch.equal(tail[4:7], body[4:7]), f"{what}: tail {tail[4:7].tolist()} body {body[4:7].tolist()}"
        assert torch.equal(tail[:4], body[:4])


# ---------------------------------------------------------------------------------------------------------------------
# the device state of pssr_adamw_step_dev
def test_adamw_dev_follows_the_state_words():
    """state[0] goes up by one per call; the lr used is the f32 in state[1], read at every call"""
    from pssr2_amd import ops
    cfg = R.CONFIGS["base"]
    n = 1027
    p0, gs, m0, v0 = R.inputs("base", n)
    p, m, v = (t.clone().cuda() for t in (p0, m0, v0))
    state = _dev_state(1, 1e-3)
    worst = [0.0, 0.0, 0.0]
    lrs = (1e-3, 0.25, 3e-5)
    for k, lr in enumerate(lrs):
        state[1] = _bits(lr)            # the word between the calls: the next step has to follow it
        h = cfg.h._replace(lr=float(np.float32(lr)))
        before = [t.double().cpu() for t in (p, m, v)]
        ops.adamw_step_dev(p, gs[k].cuda(), m, v, state, h.beta1, h.beta2, h.eps, h.wd, h.grad_scale)
        assert state.tolist() == [2 + k, _bits(lr)]
        args = (before[0], gs[k].double(), before[1], before[2])
        want, bound = R.adamw64(*args, h, 2 + k), R.adamw_bound(*args, h, 2 + k)
        r = R.ratios([t.cpu() for t in (p, m, v)], want, bound)
        assert max(r) <= 1.0, f"lr {lr}: error / bound (p, m, v) = {r}"
        # ... and a step with the lr the word held before, or with a step count that did not advance, is outside
        for wrong_h, wrong_t in ((h._replace(lr=float(np.float32(lrs[k - 1]))), 2 + k), (h, 1 + k)):
            wr = R.ratios([t.cpu() for t in (p, m, v)], R.adamw64(*args, wrong_h, wrong_t), bound)
            assert wr[0] > 1.0
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"adamw dev state words: worst error / bound (p, m, v) = {worst}")


# ---------------------------------------------------------------------------------------------------------------------
# pssr_adamw_step_amp
@pytest.mark.parametrize("n", [3, 7, 1027])
def test_adamw_amp_clear_flag_is_step_dev_with_the_scale_divided_out(n):
    from pssr2_amd import ops
    cfg = R.CONFIGS["base"]
    h = cfg.h
    p0, gs, m0, v0 = R.inputs("base", n)
    a = [t.clone().cuda() for t in (p0, m0, v0)]
    b = [t.clone().cuda() for t in (p0, m0, v0)]
    sa, sb = _dev_state(9, h.lr), _dev_state(9, h.lr)
    amp = _amp_state(scale=AMP_SCALE, good=1, skipped=2)
    for k in range(R.STEPS):
        g = gs[k].cuda()
        ops.adamw_step_amp(a[0], g, a[1], a[2], sa, h.beta1, h.beta2, h.eps, h.wd, amp, 2.0, 0.5, 1000, h.grad_scale)
        ops.adamw_step_dev(b[0], g, b[1], b[2], sb, h.beta1, h.beta2, h.eps, h.wd, h.grad_scale / AMP_SCALE)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert sa.tolist() == sb.tolist() == [10 + k, _bits(h.lr)]
        assert amp.tolist() == [_bits(AMP_SCALE), 2 + k, 2, 0]


@pytest.mark.parametrize("n", [3, 7, 1027])
def test_adamw_amp_set_flag_skips_the_step(n):
    from pssr2_amd import ops
    h = R.CONFIGS["base"].h
    p0, gs, m0, v0 = R.inputs("base", n)
    p0[0], m0[n - 1] = -0.0, float(np.float32(1e-42))         # bits that a rewrite would not keep: -0 and a subnormal
    bufs = [t.clone().cuda() for t in (p0, m0, v0)]
    g = gs[0].clone()
    g[n // 2] = float("inf")
    state = _dev_state(9, h.lr)
    amp = _amp_state(scale=AMP_SCALE, good=2, skipped=5, flag=1)
    ops.adamw_step_amp(bufs[0], g.cuda(), bufs[1], bufs[2], state, h.beta1, h.beta2, h.eps, h.wd, amp, 2.0, 0.5, 3, h.grad_scale)
    for got, was in zip(bufs, (p0, m0, v0)):
        assert torch.equal(got.cpu().view(torch.int32), was.view(torch.int32))
    assert state.tolist() == [9, _bits(h.lr)]
    assert amp.tolist() == [_bits(AMP_SCALE * 0.5), 0, 6, 0]


@pytest.mark.parametrize("growth,backoff", R.POLICIES)
def test_amp_policy_follows_the_model(growth, backoff):
    """twelve steps, finite and not, through pssr_amp_check + pssr_adamw_step_amp: scale, good-step run, skipped count, step count and
    whether the parameters moved follow the policy model (which test_optim_ref64 ties to LossScaler._step_host) exactly"""
    from pssr2_amd import ops
    h = R.CONFIGS["base"].h
    n = 1027
    p0, gs, m0, v0 = R.inputs("base", n)
    p, m, v = (t.clone().cuda() for t in (p0, m0, v0))
    state = _dev_state(0, h.lr)
    amp = _amp_state(scale=2.0 ** 12)
    model = R.Scaler(np.float32(2.0 ** 12), 0, 0)
    steps = 0
    for i, finite in enumerate(R.FINITE_SEQUENCE):
        g = gs[i % R.STEPS].clone() * float(model.scale)
        if not finite:
            g[(37 * i) % n] = float("inf") if i % 2 else float("nan")
        g = g.cuda()
        was = [t.clone() for t in (p, m, v)]
        ops.amp_check(g, amp)
        assert amp.tolist() == [_bits(float(model.scale)), model.good, model.skipped, int(not finite)]
        ops.adamw_step_amp(p, g, m, v, state, h.beta1, h.beta2, h.eps, h.wd, amp, growth, backoff, R.INTERVAL, h.grad_scale)
        model = R.scaler_step(model, finite, growth, backoff, R.INTERVAL)
        steps += int(finite)
        assert amp.tolist() == [_bits(float(model.scale)), model.good, model.skipped, 0], f"step {i}"
        assert int(state[0]) == steps
        moved = [not torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((p, m, v), was)]
        assert moved == [finite] * 3, f"step {i}: finite={finite}, (p, m, v) moved: {moved}"
    assert (model.good, model.skipped, steps) == (0, 3, 9)


# ---------------------------------------------------------------------------------------------------------------------
# pssr_amp_check
CHECK_BIG = 4 * 256 * 2048 + 4096 + 3       # the 2048 workgroups of amp_check_kernel make a second trip; a body remainder and a tail
NONFINITE = {"+inf": 0x7F800000, "-inf": 0xFF800000, "quiet nan": 0x7FC00000, "nan, smallest mantissa": 0x7F800001,
             "nan, sign set": 0xFFC00001}
AMP_WORDS = [_bits(4096.0), 5, 7]


def _i32(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


def _positions(n):
    n4 = n // 4 * 4
    pos = {0, n - 1} | set(range(n4, n))
    if n4:
        pos.add(n4 - 1)
    if n > 4 * 256 * 2048:
        pos.add(4 * 256 * 2048)
    return sorted(pos)


@pytest.mark.parametrize("n", [1, 3, 4, 7, 1027, CHECK_BIG])
def test_amp_check_finds_one_nonfinite_value_anywhere(n):
    from pssr2_amd import ops
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
    gi = g.view(torch.int32)
    for pos in _positions(n):
        keep = int(gi[pos])
        for kind, bits in NONFINITE.items():
            gi[pos] = _i32(bits)
            amp = torch.tensor(AMP_WORDS + [0], dtype=torch.int32, device="cuda")
            ops.amp_check(g, amp)
            assert amp.tolist() == AMP_WORDS + [1], f"n={n}: {kind} at {pos} -> {amp.tolist()}"
        gi[pos] = keep
    amp = torch.tensor(AMP_WORDS + [0], dtype=torch.int32, device="cuda")
    ops.amp_check(g, amp)
    assert amp.tolist() == AMP_WORDS + [0], "the buffer was not restored, or a finite value raised the flag"


@pytest.mark.parametrize("n", [1, 3, 4, 7, 1027, CHECK_BIG])
def test_amp_check_leaves_the_flag_on_finite_input(n):
    from pssr2_amd import ops
    finite = [0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x80000000, 0x00000000, 0x7F000000, 0x00800000]   # +-FLT_MAX, subnormals, -0 ...
    pattern = torch.tensor([_i32(b) for b in finite], dtype=torch.int32)
    for g in (pattern.repeat(n // 8 + 1)[:n].clone().view(torch.float32), torch.zeros(n)):
        g = g.cuda()
        for flag in (0, 1):             # the check only ORs: a flag that is set stays set
            amp = torch.tensor(AMP_WORDS + [flag], dtype=torch.int32, device="cuda")
            ops.amp_check(g, amp)
            assert amp.tolist() == AMP_WORDS + [flag]


# ---------------------------------------------------------------------------------------------------------------------
# alignment
def test_every_entry_point_refuses_a_misaligned_buffer_of_four_or_more():
    """the float4 body needs 16-byte aligned buffers: a view at a 4-byte offset with n >= 4 raises and launches nothing"""
    from pssr2_amd import ops
    h = R.CONFIGS["base"].h
    n = 8
    big = [torch.randn(n + 4, generator=torch.Generator().manual_seed(i)).cuda() for i in range(4)]
    for which in range(4):              # each of p, g, m, v in turn is the misaligned one
        views = [t[1:n + 1] if i == which else t[:n] for i, t in enumerate(big)]
        assert views[which].data_ptr() % 16 == 4
        p, g, m, v = views
        was = [t.clone() for t in big]
        state, amp = _dev_state(3, h.lr), _amp_state(flag=0)
        with pytest.raises(RuntimeError, match="aligned"):
            ops.adamw_step(p, g, m, v, h.lr, h.beta1, h.beta2, h.eps, h.wd, 4, h.grad_scale)
        with pytest.raises(RuntimeError, match="aligned"):
            ops.adamw_step_dev(p, g, m, v, state, h.beta1, h.beta2, h.eps, h.wd, h.grad_scale)
        with pytest.raises(RuntimeError, match="aligned"):
            ops.adamw_step_amp(p, g, m, v, state, h.beta1, h.beta2, h.eps, h.wd, amp, 2.0, 0.5, 3, h.grad_scale)
        torch.cuda.synchronize()
        assert state.tolist() == [3, _bits(h.lr)] and amp.tolist() == [_bits(AMP_SCALE), 0, 0, 0]
        for t, w in zip(big, was):
            assert torch.equal(t.view(torch.int32), w.view(torch.int32))
    g = big[1][1:n + 1]
    g[2] = float("inf")
    amp = _amp_state(flag=0)
    with pytest.raises(RuntimeError, match="amp_check"):
        ops.amp_check(g, amp)
    torch.cuda.synchronize()
    assert amp.tolist() == [_bits(AMP_SCALE), 0, 0, 0]
