"""ops.window_attn_fwd / window_attn_bwd (csrc/window_attn.hip) against a float64 restatement of WindowAttention with the cyclic
shift, the window partition and the attention mask, written here with torch ops on the CPU.

Yardstick: the same restatement run on the device in the kernel's storage dtype (every tensor, S and P included, in that dtype)
against the same float64 truth; for bfloat16 the truth is computed from the bf16-rounded inputs.  Errors are max |x - truth| /
max |truth| per tensor.  The kernel may be at most 4x the composition's error in float32 (two float32 evaluations with different
summation orders) and at most 2x in bfloat16 (the composition rounds S and P to bf16, the kernel keeps them in float32 and so should
sit below 1x; the factor leaves room for a bf16 P operand in P v)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, H, W, heads, hd, ws, shift)
SHAPES = [(2, 16, 24, 2, 16, 8, 4), (2, 16, 24, 2, 16, 8, 0), (1, 12, 12, 3, 10, 4, 2), (1, 8, 16, 1, 32, 8, 3), (2, 6, 9, 2, 5, 3, 1),
          (1, 8, 8, 6, 30, 8, 0)]
FACTOR = {torch.float32: 4.0, torch.bfloat16: 2.0}


def _mask(h, w, ws, shift):
    """[nW, N, N] as SwinTransformerBlock.calculate_mask: region ids painted with slices, partitioned, compared."""
    img = torch.zeros(h, w, dtype=torch.float64)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    ids = img.view(h // ws, ws, w // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    diff = ids[:, None, :] - ids[:, :, None]
    return torch.where(diff != 0, -100.0, 0.0)


def attention(qkv, bias_table, heads, ws, shift, scale):
    """(out [B, H, W, C], lse [B, heads, H, W]) in qkv's dtype, differentiable: roll, partition, q k^T, bias, mask, softmax, P v,
    reverse, roll back."""
    b, h, w, c3 = qkv.shape
    c, n, nh, nw = c3 // 3, ws * ws, h // ws, w // ws
    x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    win = x.view(b, nh, ws, nw, ws, c3).permute(0, 1, 3, 2, 4, 5).reshape(b * nh * nw, n, 3, heads, c // heads)
    q, k, v = win.permute(2, 0, 3, 1, 4).unbind(0)
    s = (q * scale) @ k.transpose(-2, -1)
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    ys, xs = ys.flatten().to(qkv.device), xs.flatten().to(qkv.device)
    index = (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)
    s = s + bias_table.to(qkv.dtype)[index.view(-1)].view(n, n, heads).permute(2, 0, 1)
    if shift:
        s = (s.view(b, nh * nw, heads, n, n) + _mask(h, w, ws, shift).to(qkv.device, qkv.dtype)[None, :, None]).view(-1, heads, n, n)
    p = torch.softmax(s, dim=-1)
    lse = torch.logsumexp(s, dim=-1)                                             # [B nW, heads, N]
    o = (p @ v).transpose(1, 2).reshape(b, nh, nw, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)
    lse = lse.view(b, nh, nw, heads, ws, ws).permute(0, 3, 1, 4, 2, 5).reshape(b, heads, h, w)
    if shift:
        o, lse = torch.roll(o, (shift, shift), (1, 2)), torch.roll(lse, (shift, shift), (2, 3))
    return o, lse


def _run(fn_inputs, dtype, device):
    qkv, bias, dout, heads, ws, shift, scale = fn_inputs
    q = qkv.to(device, dtype).requires_grad_(True)
    bt = bias.to(device, torch.float64 if dtype == torch.float64 else torch.float32).requires_grad_(True)
    out, lse = attention(q, bt, heads, ws, shift, scale)
    (out * dout.to(device, dtype)).sum().backward()
    return [t.detach().double().cpu() for t in (out, lse, q.grad, bt.grad)]


@functools.lru_cache(maxsize=None)
def case(shape, dtype, q_mul=1.0):
    """Inputs (rounded to the storage dtype), the float64 truth and the device composition's errors; made once per case."""
    b, h, w, heads, hd, ws, shift = shape
    g = torch.Generator().manual_seed(hash((shape, q_mul)) % (1 << 31))
    c = heads * hd
    qkv = torch.randn(b, h, w, 3 * c, generator=g)
    qkv[..., :c] *= q_mul
    qkv = qkv.to(dtype).float()
    bias = 0.5 * torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    dout = torch.randn(b, h, w, c, generator=g).to(dtype).float()
    inputs = (qkv, bias, dout, heads, ws, shift, hd ** -0.5)
    truth = _run(inputs, torch.float64, "cpu")
    comp = _run(inputs, dtype, "cuda")
    return inputs, truth, [err(c_, t_) for c_, t_ in zip(comp, truth)]


def err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def kernel(inputs, dtype):
    from pssr2_amd import ops
    qkv, bias, dout, heads, ws, shift, scale = inputs
    q, bt, do = qkv.cuda().to(dtype), bias.cuda(), dout.cuda().to(dtype)
    out, lse = ops.window_attn_fwd(q, bt, heads, ws, shift, scale)
    dqkv, dbias = ops.window_attn_bwd(q, bt, lse, do, heads, ws, shift, scale)
    assert out.dtype == dtype and dqkv.dtype == dtype and lse.dtype == torch.float32 and dbias.dtype == torch.float32
    return [t.double().cpu() for t in (out, lse, dqkv, dbias)]


def check(shape, dtype, q_mul=1.0):
    inputs, truth, comp_err = case(shape, dtype, q_mul)
    got = kernel(inputs, dtype)
    for name, g, t, ce in zip(("out", "lse", "dqkv", "dbias_table"), got, truth, comp_err):
        assert torch.isfinite(g).all(), name
        e = err(g, t)
        print(f"{shape} {dtype} x{q_mul:g} {name}: kernel {e:.3g}, composition {ce:.3g}")
        assert e <= FACTOR[dtype] * ce, (name, e, ce)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward(shape, dtype):
    check(shape, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_masked_entries_are_added_not_dropped(dtype):
    """q x 40: the unmasked logits of a row spread over more than 100, so entries masked with -100 keep weight in the softmax."""
    shape = SHAPES[0]
    inputs, truth, _ = case(shape, dtype, 40.0)
    qkv, bias, _, heads, ws, shift, scale = inputs
    # the premise, on the truth's side: some masked logit lies above some unmasked logit of its row
    s = _logits(qkv.double(), bias.double(), heads, ws, shift, scale)
    masked = _mask(shape[1], shape[2], ws, shift)[None, :, None] != 0
    spread = (s.masked_fill(masked, float("-inf")).amax(-1) - s.masked_fill(masked, float("inf")).amin(-1)).max()
    assert spread > 100, float(spread)
    check(shape, dtype, 40.0)


def _logits(qkv, bias, heads, ws, shift, scale):
    """q k^T scale + bias without the mask, [B, nW, heads, N, N], float64."""
    b, h, w, c3 = qkv.shape
    n = ws * ws
    x = torch.roll(qkv, (-shift, -shift), (1, 2))
    win = x.view(b, h // ws, ws, w // ws, ws, c3).permute(0, 1, 3, 2, 4, 5).reshape(-1, n, 3, heads, c3 // 3 // heads)
    q, k, _ = win.permute(2, 0, 3, 1, 4).unbind(0)
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    ys, xs = ys.flatten(), xs.flatten()
    index = (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)
    s = (q * scale) @ k.transpose(-2, -1) + bias[index.view(-1)].view(n, n, heads).permute(2, 0, 1)
    return s.view(b, -1, heads, n, n)


def test_backward_is_bit_reproducible():
    from pssr2_amd import ops
    inputs, _, _ = case(SHAPES[0], torch.float32)
    qkv, bias, dout, heads, ws, shift, scale = inputs
    q, bt, do = qkv.cuda(), bias.cuda(), dout.cuda()
    out, lse = ops.window_attn_fwd(q, bt, heads, ws, shift, scale)
    first = ops.window_attn_bwd(q, bt, lse, do, heads, ws, shift, scale)
    second = ops.window_attn_bwd(q, bt, lse, do, heads, ws, shift, scale)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert torch.equal(out, ops.window_attn_fwd(q, bt, heads, ws, shift, scale)[0])


def test_argument_errors():
    from pssr2_amd import _lib as L
    from pssr2_amd import ops

    def call(b, h, w, heads, hd, ws, shift):
        qkv = torch.zeros(b, h, w, 3 * heads * hd, device="cuda")
        return ops.window_attn_fwd(qkv, torch.zeros((2 * ws - 1) ** 2, heads, device="cuda"), heads, ws, shift, 1.0)

    call(1, 8, 8, 2, 32, 8, 7)                                                   # the largest shapes taken
    for args, word in (((1, 8, 8, 2, 33, 8, 0), "head dim"), ((1, 9, 9, 1, 8, 9, 0), "window size"), ((1, 8, 8, 1, 8, 8, 8), "shift"),
                       ((1, 8, 12, 1, 8, 8, 0), "multiples")):
        with pytest.raises(RuntimeError, match=r"\(-1\).*" + word):
            call(*args)
    lib = L.lib()
    buf = torch.zeros(8 * 8 * 48, device="cuda")
    assert lib.pssr_window_attn_fwd(None, L.ptr(buf), L.ptr(buf), L.ptr(buf), 1, 8, 8, 16, 1, 8, 0, 1.0, L.F32, None) == -1
    assert b"null" in lib.pssr_last_error()
    assert lib.pssr_window_attn_bwd(L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), None, 0, 1, 8, 8, 16, 1, 8, 0, 1.0,
                                    L.F32, None) == -1
    assert b"null" in lib.pssr_last_error()
    assert lib.pssr_window_attn_bwd(L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), 16, 1, 8, 8, 16, 1, 8, 0,
                                    1.0, L.F32, None) == -1
    assert b"workspace" in lib.pssr_last_error()
    assert lib.pssr_window_attn_fwd(L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), 1, 8, 8, 16, 3, 8, 0, 1.0, L.F32, None) == -1
    assert b"multiple of heads" in lib.pssr_last_error()
    assert lib.pssr_window_attn_fwd(L.ptr(buf), L.ptr(buf), L.ptr(buf), L.ptr(buf), 1, 8, 8, 16, 1, 8, 0, 1.0, L.F16, None) == -1
