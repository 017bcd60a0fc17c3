"""Dense head-dimension-48 cross-attention (csrc/dense_attn.hip through include/transoar_denseattn.h) against plain
torch in fp64 on the bf16-rounded inputs: softmax(scale q k^T, masked) v per 48-column head, gradients from autograd.
Bound: the bf16-storage rule (README "How parity is stated"), max|a - b| / max|b| <= 2^-7 on O, dQ, dK, dV; lse to 1e-4."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
H, HD, C = 8, 48, 384
SCALE = HD ** -0.5


def _windows(n_keys):
    """Live key windows [lo, hi) whose ends fall inside a 32-key word: nearly everything; 7 keys (less than a tile); the
    middle third; the last 7 keys only (the leading tiles are skipped); keys 1..8 only (the trailing tiles are)."""
    return [(3, n_keys - 5), (n_keys // 2 + 1, n_keys // 2 + 8), (n_keys // 3, 2 * (n_keys // 3) + 3), (n_keys - 7, n_keys), (1, 9)]


@functools.lru_cache(maxsize=None)
def _case(b, n_q, n_keys, masked):
    """-> bf16 inputs on the GPU, the boolean mask (or None) and the fp64 reference (o, lse, dq, dk, dv), computed once."""
    g = torch.Generator().manual_seed(n_q + n_keys)
    q, k, v, d_o = (torch.randn(b, n, C, generator=g).to(torch.bfloat16) for n in (n_q, n_keys, n_keys, n_q))
    mask = None
    if masked:
        n_org = 5 if n_q % 5 == 0 else 9          # 27 queries cannot be 5 organs: 9 organs of 3, the five windows in turn
        mask = torch.ones(n_q, n_keys, dtype=torch.bool)
        rows = n_q // n_org
        for o in range(n_org):
            lo, hi = _windows(n_keys)[o % 5]
            mask[o * rows:(o + 1) * rows, lo:hi] = False
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    heads = lambda t: t.view(b, -1, H, HD).transpose(1, 2)          # noqa: E731
    s = SCALE * heads(q64) @ heads(k64).transpose(-1, -2)
    if masked:
        s = s.masked_fill(mask, float("-inf"))
    o = (torch.softmax(s, -1) @ heads(v64)).transpose(1, 2).reshape(b, n_q, C)
    o.backward(d_o.double())
    ref = (o.detach(), torch.logsumexp(s, -1).detach(), q64.grad, k64.grad, v64.grad)
    return tuple(t.cuda() for t in (q, k, v, d_o)), (mask.cuda() if masked else None, n_org if masked else 1), ref


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape,split", [((1, 27, 50), None), ((2, 135, 200), None), ((1, 405, 1000), 1), ((1, 405, 1000), 3)])
def test_dense_attention_matches_fp64(shape, split, masked):
    from transoar_amd import dense_attn
    (q, k, v, d_o), (mask, n_org), ref = _case(*shape, masked)
    assert dense_attn.usable(q, k, v, H)
    bits = dense_attn.key_bits(mask, n_org) if masked else None
    runs = []
    for _ in range(2):
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        out, lse = dense_attn.dense_attention(qg, kg, vg, bits, SCALE, split, return_lse=True)
        out.backward(d_o)
        runs.append((out.detach(), lse, qg.grad, kg.grad, vg.grad))
    torch.cuda.synchronize()
    errs = {n: _rel(runs[0][i], ref[i]) for i, n in ((0, "o"), (2, "dq"), (3, "dk"), (4, "dv"))}
    lse_err = float((runs[0][1].double().cpu() - ref[1]).abs().max())
    print(shape, split, masked, errs, lse_err)
    assert max(errs.values()) <= 2.0 ** -7, errs
    assert lse_err <= 1e-4, lse_err
    # dK / dV are owned by one workgroup per key block (no atomics): bit-equal from run to run
    assert torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][4], runs[1][4])
    if masked:          # keys no organ may see receive exactly zero
        dead = mask.all(0)
        assert float(runs[0][3][:, dead].abs().max()) == 0.0 and float(runs[0][4][:, dead].abs().max()) == 0.0


@pytest.mark.parametrize("what", ["all_masked_organ", "channels", "rows_per_organ"])
def test_refusals_launch_nothing(what):
    """The binding refuses an organ without a key; the library returns TRANSOAR_DENSEATTN_ERR_DIM (-2) before its
    first HIP call (the pointers are host addresses: a launch would fault)."""
    from transoar_amd import dense_attn
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    fwd = dense_attn.lib.transoar_dense_attn_forward
    if what == "all_masked_organ":
        mask = torch.zeros(10, 50, dtype=torch.bool).cuda()
        mask[4:6] = True
        with pytest.raises(ValueError, match="no key"):
            dense_attn.key_bits(mask, 5)
    elif what == "channels":
        q = torch.zeros(1, 27, 256, dtype=torch.bfloat16).cuda()
        assert not dense_attn.usable(q, q, q, H)
        assert fwd(p, p, p, None, None, p, p, None, 0, 1, 27, 50, 256, H, 1, 27, SCALE, 1, None) == -2
    else:
        assert fwd(p, p, p, p, p, p, p, None, 0, 1, 27, 50, C, H, 5, 6, SCALE, 1, None) == -2          # 27 % 6 != 0
        assert dense_attn.lib.transoar_dense_attn_backward(p, p, p, p, p, p, p, p, p, p, p, p, 1 << 20, 1, 27, 50, C, H, 5, 6,
                                                           SCALE, 1, None) == -2
