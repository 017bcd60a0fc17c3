"""FocusedDecoderLayer whose cross-attention takes the dense branch (restrict_attn False; boxes too large to gather)
under bf16 autocast on the fused kernels (csrc/dense_attn.hip), against the same layer in fp64 on the CPU.

Bound: 2 x the largest error the torch route it replaces (TRANSOAR_DENSE_FUSED=0: F.scaled_dot_product_attention with
the additive mask) shows against the same fp64 result on the MI355X -- DESIGN.md section 12.13 records the three
errors per case; both routes are bf16-storage flash attentions that differ in summation order only."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

# largest of (output, d src, d tgt) of the torch route on the MI355X, per case
TORCH_ROUTE_ERROR = {False: 0.0151711, True: 0.0175431}


def _layer(restrict):
    from transoar_amd.focused_decoder import FocusedDecoderLayer
    n_org = 20
    config = {"num_queries": 7 * n_org, "num_organs": n_org, "input_levels": "P5", "restrict_attn": restrict}          # 5 x 5 x 8 tokens
    props = {str(i): {"attn_area": [0.05 * (i % 4), 0.0, 0.02 * i, 1.0 - 0.05 * (i % 3), 1.0, 0.9]} for i in range(n_org)}
    torch.manual_seed(3)
    layer = FocusedDecoderLayer(384, 256, 0.1, "relu", 8, config, props).eval()
    assert not layer._use_roi and bool(layer.attn_mask.any()) == restrict
    return layer


def layer_errors(restrict):
    """-> (relative errors of the output, d src and d tgt against fp64 on the CPU; the GPU layer)"""
    layer = _layer(restrict)
    g = torch.Generator().manual_seed(5)
    tgt, query_pos = torch.randn(2, 140, 384, generator=g), torch.randn(2, 140, 384, generator=g)
    src, src_pos = torch.randn(2, 200, 384, generator=g), torch.randn(2, 200, 384, generator=g)
    d_out = torch.randn(2, 140, 384, generator=g)

    def run(mod, cast, autocast):
        t, s = cast(tgt).requires_grad_(True), cast(src).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = mod(t, cast(query_pos), cast(src_pos), s)[0]
        out.backward(cast(d_out))
        return [x.detach().double().cpu() for x in (out, s.grad, t.grad)]

    ref = run(copy.deepcopy(layer).double(), lambda x: x.double(), False)
    gpu = layer.cuda()
    got = run(gpu, lambda x: x.cuda(), True)
    return [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, ref)], gpu


@pytest.mark.parametrize("restrict", [False, True])
def test_dense_branch_on_the_fused_kernels_matches_fp64(restrict):
    from transoar_amd import dense_attn
    assert dense_attn.ENABLED
    errs, layer = layer_errors(restrict)
    print(restrict, errs)
    assert max(errs) <= 2 * TORCH_ROUTE_ERROR[restrict], errs
    assert layer._attn_bias is None          # the dense additive mask was never built
