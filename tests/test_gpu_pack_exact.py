"""Bit-exact tests of the weight pack (csrc/pack.hip: pssr_pack_conv_weight, pssr_pack_conv_weight_batch) on its own: no
convolution involved.

The reference (tests/_conv_exact.py: pack_map, pack_reference) is written from the layout documented in include/pssr_mi355.h and
checked on the CPU in tests/test_conv_exact_helpers.py -- against unpack_map for the forward forms, against
torch.nn.grad.conv2d_input for the transposed ones -- where the comparison helper is also shown to report a dropped slot swizzle, a
truncating conversion, -0 or unwritten padding and unflipped taps.  Every case here
  * packs seeded normal f32 values with edge values at known places (ties of the storage type in both directions, -0, the smallest
    subnormal and the largest finite number, the float16 overflow boundary, f32 subnormals) into a destination pre-filled with 0xFF,
  * requires the whole buffer of pssr_packed_weight_bytes to equal the reference bytewise: every byte written, padding +0,
  * repeats that with NaN in every source element outside the channel window, and
  * packs another weight into the same buffer and requires equality again.
The case table is tests/_pack_cases.py."""
import pytest
import torch

import _pack_cases as P
from _conv_exact import assert_packed_equal

pytestmark = pytest.mark.gpu


def _code(dt):
    from pssr2_amd import ops
    return ops.dtype_code(dt)


def _bytes(name, dt):
    from pssr2_amd import _lib as L
    taps, k_pad, n_pad = P.geometry(name)
    nbytes = L.lib().pssr_packed_weight_bytes(taps, k_pad, n_pad, _code(dt))
    assert nbytes == taps * k_pad * n_pad * torch.empty(0, dtype=dt).element_size()
    return nbytes


def _dest(name, dt):
    """a PackedWeight over a 0xFF-filled buffer of exactly pssr_packed_weight_bytes"""
    from pssr2_amd import ops
    taps, k_pad, n_pad = P.geometry(name)
    return ops.PackedWeight(torch.full((_bytes(name, dt),), 0xFF, dtype=torch.uint8, device="cuda"), taps, k_pad, n_pad, _code(dt))


def _perm_dev(name):
    perm = P.perm_of(name)
    return None if perm is None else perm.to(torch.int32).cuda()


def _single(name, dt, w, out=None):
    """pssr_pack_conv_weight of a (non-centre) case into `out` (a fresh 0xFF-filled buffer if None)"""
    from pssr2_amd import ops
    c = P.EVERY[name]
    out = _dest(name, dt) if out is None else out
    res = ops.pack_conv_weight(w.cuda(), _code(dt), mode=c["mode"], ci_begin=c["ci_begin"], ci_count=c["ci_count"], n_perm=_perm_dev(name),
                               out=out)
    assert res is out and (out.taps, out.k_pad, out.n_pad) == P.geometry(name)
    return out


def _no_nan(buf, dt, what):
    assert not bool(buf.view(dt).float().isnan().any()), f"{what}: a NaN from outside the channel window arrived"


@pytest.mark.parametrize("name,dt", [(n, dt) for n, c in P.CASES.items() for dt in c["dtypes"]], ids=lambda v: P.DT_NAME.get(v, v))
def test_pack_single(name, dt):
    taps, _, n_pad = P.geometry(name)
    pmap = P.case_map(name, dt)
    w = P.source(name, dt, pmap=pmap)
    want = P.reference(name, dt, w, pmap)
    out = _single(name, dt, w)
    assert_packed_equal(out.data, want, taps, n_pad, f"{name} {dt}")
    # the same values inside the window, NaN in every source element outside it
    wn = P.source(name, dt, nan_outside=True, pmap=pmap)
    out_n = _single(name, dt, wn)
    _no_nan(out_n.data, dt, name)
    assert_packed_equal(out_n.data, want, taps, n_pad, f"{name} {dt} (NaN outside the window)")
    # another weight into the buffer that holds the first: nothing stale may survive
    w2 = P.source(name, dt, variant=1, pmap=pmap)
    _single(name, dt, w2, out=out)
    assert_packed_equal(out.data, P.reference(name, dt, w2, pmap), taps, n_pad, f"{name} {dt} (second pack into the same buffer)")


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def _raw_pack(w, dst, cout, cin, ks, ci_begin, ci_count, mode, k_pad, n_pad, dtype):
    from pssr2_amd import _lib as L
    return L.lib().pssr_pack_conv_weight(L.ptr(w), L.ptr(dst), cout, cin, ks, ci_begin, ci_count, mode, None, k_pad, n_pad, dtype,
                                         L.stream_ptr())


REFUSALS = {    # (cout, cin, ks, ci_begin, ci_count, mode, k_pad, n_pad, dtype code)
    "ks4": (16, 16, 4, 0, 16, 0, 16, 128, 1),
    "mode6": (16, 16, 3, 0, 16, 6, 16, 128, 1),
    "ks2_mode0": (16, 16, 2, 0, 16, 0, 16, 128, 1),
    "window_past_cin": (16, 16, 3, 8, 9, 0, 16, 128, 1),
    "k_pad_below_gemm_k": (16, 32, 3, 0, 32, 0, 16, 128, 1),
    "n_pad_96": (16, 16, 3, 0, 16, 0, 16, 96, 1),
    "dtype7": (16, 16, 3, 0, 16, 0, 16, 128, 7),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_pack_refuses(name):
    from pssr2_amd import _lib as L
    cout, cin, ks, b, c, mode, k_pad, n_pad, code = REFUSALS[name]
    w = torch.randn(cout, cin, ks, ks, device="cuda")
    dst = torch.full((9 * 32 * 128 * 4,), 0xFF, dtype=torch.uint8, device="cuda")        # room for any of the above in any type
    status = _raw_pack(w, dst, cout, cin, ks, b, c, mode, k_pad, n_pad, code)
    torch.cuda.synchronize()
    assert status != 0, f"{name}: accepted"
    with pytest.raises(RuntimeError, match="pack"):
        L.check(status, "pssr_pack_conv_weight")
    assert bool((dst == 0xFF).all()), f"{name}: refused, but the destination was written"


def test_pack_accepts_what_the_refusals_are_derived_from():
    """the refused calls differ from this accepted one in one argument each"""
    w = torch.randn(16, 16, 3, 3, device="cuda")
    dst = torch.full((9 * 16 * 128 * 2,), 0xFF, dtype=torch.uint8, device="cuda")
    assert _raw_pack(w, dst, 16, 16, 3, 0, 16, 0, 16, 128, 1) == 0
    torch.cuda.synchronize()
    assert not bool((dst.view(torch.int16) == -1).any())       # 0xFFFF is a bf16 NaN: no element of the pre-fill is left


# ---------------------------------------------------------------------------------------------------------------------
# the batch entry point
def _item(name, dt, w_dev, dst, perm_dev):
    """pssr_pack_item of a case, filled as _Conv.item (pssr2_amd/engine.py) fills it"""
    from pssr2_amd import _lib as L
    c = P.EVERY[name]
    _, k_pad, n_pad = P.geometry(name)
    it = L.PackItem()
    it.w, it.packed = w_dev.data_ptr(), dst.data_ptr()
    it.n_perm = perm_dev.data_ptr() if perm_dev is not None else None
    it.cout, it.cin, it.ks = c["cout"], c["cin"], c["ks"]
    it.ci_begin, it.ci_count = c["ci_begin"], c["ci_count"]
    it.mode, it.k_pad, it.n_pad, it.dtype, it.center = c["mode"], k_pad, n_pad, _code(dt), int(c["center"])
    return it


def _table(items):
    from pssr2_amd import _lib as L
    arr = (L.PackItem * len(items))(*items)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _batch(table, n_items):
    from pssr2_amd import _lib as L
    return L.lib().pssr_pack_conv_weight_batch(L.ptr(table), n_items, L.stream_ptr())


def _run_batch(entries):
    """entries: [(name, dt, source on the host)].  One launch; returns the destinations (0xFF-filled before the launch)."""
    from pssr2_amd import _lib as L
    keep, items, dsts = [], [], []
    for name, dt, w in entries:
        w_dev, perm_dev = w.cuda(), _perm_dev(name)
        dst = torch.full((_bytes(name, dt),), 0xFF, dtype=torch.uint8, device="cuda")
        keep += [w_dev, perm_dev]
        dsts.append(dst)
        items.append(_item(name, dt, w_dev, dst, perm_dev))
    table = _table(items)
    L.check(_batch(table, len(items)), "pssr_pack_conv_weight_batch")
    torch.cuda.synchronize()
    return dsts


def test_pack_batch_every_case_in_one_launch():
    """all the single-launch cases, storage types and modes interleaved, in one batch: each destination equals the reference and
    the single pack of the same weight bytewise"""
    entries = [(n, dt, P.source(n, dt, nan_outside=True)) for n, c in P.CASES.items() for dt in c["dtypes"]]
    entries.sort(key=lambda e: P.stable_seed(e[0], P.DT_NAME[e[1]]))        # mixed: neighbours differ in type, mode and path
    assert len(entries) >= 40
    for (name, dt, w), dst in zip(entries, _run_batch(entries)):
        taps, _, n_pad = P.geometry(name)
        what = f"batch item {name} {dt}"
        _no_nan(dst, dt, what)
        assert_packed_equal(dst, P.reference(name, dt, w), taps, n_pad, what)
        assert torch.equal(dst, _single(name, dt, w).data), f"{what}: differs from the single pack"


def test_pack_batch_of_one_item():
    name, dt = "t33_m0_all", torch.bfloat16
    w = P.source(name, dt)
    taps, _, n_pad = P.geometry(name)
    assert_packed_equal(_run_batch([(name, dt, w)])[0], P.reference(name, dt, w), taps, n_pad, name)


@pytest.mark.parametrize("name", list(P.CENTER))
def test_pack_batch_centre_items(name):
    """a [cout, cin, 1, 1] source packed as the centre tap of a 3x3 kernel equals the single pack of the zero-stuffed 3x3 weight
    (what _Conv.get packs on the lazy path) and the reference"""
    from pssr2_amd import ops
    c = P.EVERY[name]
    taps, _, n_pad = P.geometry(name)
    entries = [(name, dt, P.source(name, dt, nan_outside=True)) for dt in P.ALL]
    for (_, dt, w1), dst in zip(entries, _run_batch(entries)):
        what = f"{name} {dt}"
        _no_nan(dst, dt, what)
        assert_packed_equal(dst, P.reference(name, dt, w1), taps, n_pad, what)
        w3 = torch.zeros(c["cout"], c["cin"], 3, 3)
        w3[:, :, 1, 1] = w1[:, :, 0, 0]
        lazy = ops.pack_conv_weight(w3.cuda(), _code(dt), mode=c["mode"], ci_begin=c["ci_begin"], ci_count=c["ci_count"],
                                    n_perm=_perm_dev(name), out=_dest(name, dt))
        assert torch.equal(dst, lazy.data), f"{what}: the centre form differs from the pack of the zero-stuffed weight"


@pytest.mark.parametrize("name,dt", [(n, dt) for n, c in P.BIG.items() for dt in c["dtypes"]], ids=lambda v: P.DT_NAME.get(v, v))
def test_pack_batch_later_trips(name, dt):
    """items with more work than the 384 workgroups of a batch item cover in one trip: the loops over the tiles (pack_tiles33) and
    over the elements (pack_elems) go round again"""
    c = P.EVERY[name]
    taps, k_pad, n_pad = P.geometry(name)
    kch = 8 if dt == torch.float32 else 16
    if c["ks"] == 3:
        assert (k_pad // kch) * (n_pad // 128) > 384
    else:
        assert taps * k_pad * n_pad > 384 * 256
    pmap = P.case_map(name, dt)
    w = P.source(name, dt, pmap=pmap)
    want = P.reference(name, dt, w, pmap)
    del pmap
    dst = _run_batch([(name, dt, w)])[0]
    assert_packed_equal(dst, want, taps, n_pad, f"{name} {dt}")
    assert torch.equal(dst, _single(name, dt, w).data), f"{name}: differs from the single pack"


@pytest.mark.parametrize("n_items", [0, 65536, -1])
def test_pack_batch_refuses_item_counts(n_items):
    name, dt = "t33_m0", torch.bfloat16
    w_dev = P.source(name, dt).cuda()
    dst = torch.full((_bytes(name, dt),), 0xFF, dtype=torch.uint8, device="cuda")
    table = _table([_item(name, dt, w_dev, dst, None)])
    assert _batch(table, n_items) != 0
    assert _batch(None, 1) != 0
    torch.cuda.synchronize()
    assert bool((dst == 0xFF).all()), "refused, but an item was packed"


# ---------------------------------------------------------------------------------------------------------------------
# the engine's cache after batched re-packs
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_engine_cache_equals_fresh_packs_after_batched_repack(dt):
    """after optimizer steps, every packed buffer the engine holds -- re-packed by the one batch launch of Engine._repack_all --
    equals a fresh single pack of the current parameter bytewise, the centre forms of the first block's 1x1 residual included"""
    from pssr2_amd import ops
    from pssr2_amd.models import ResUNet
    from pssr2_amd.optim import FusedAdamW
    torch.manual_seed(5)
    model = ResUNet(hidden=[16, 32], depth=1).cuda().train()
    model.compute_dtype = dt
    code = ops.dtype_code(dt)
    eng = model._engine
    x = torch.rand(2, 1, 16, 16, device="cuda") * 255
    target = torch.rand(2, 1, 64, 64, device="cuda")
    opt = FusedAdamW(model.parameters(), lr=1e-2)
    for _ in range(2):
        torch.nn.functional.mse_loss(model(x) / 255, target).backward()
        opt.step()
    convs = list(eng._convs.values())
    stale = [(c, key) for c in convs for key in c.packed if key[1] == code and c.version.get(key) != c.ver()]
    assert len(stale) >= 8, f"only {len(stale)} stale forms: the batched path was not taken"
    forms = {(c.specs[key[0]]["mode"], bool(c.specs[key[0]].get("center"))) for c, key in stale}
    assert (2, True) in forms and (3, True) in forms, "no block with the FWD_CENTER / DGRAD_CENTER forms"
    before = {(id(c), key): c.packed[key].data.data_ptr() for c, key in stale}
    eng._repack_all(code)
    torch.cuda.synchronize()
    checked = 0
    for c in convs:
        for key, pw in c.packed.items():
            if key[1] != code:
                continue
            assert c.version[key] == c.ver() and pw.data.data_ptr() == before.get((id(c), key))     # re-packed in place by the batch
            spec = c.specs[key[0]]
            fresh = ops.pack_conv_weight(c.weight_for(spec).contiguous(), code, mode=spec["mode"], ci_begin=spec.get("ci_begin", 0),
                                         ci_count=spec.get("ci_count"), n_perm=spec.get("n_perm"))
            assert (fresh.taps, fresh.k_pad, fresh.n_pad) == (pw.taps, pw.k_pad, pw.n_pad)
            assert torch.equal(pw.data, fresh.data), f"cached form {key[0][:5]} of a {tuple(c.m.weight.shape)} weight differs from a fresh pack"
            checked += 1
    assert checked == len(stale)
