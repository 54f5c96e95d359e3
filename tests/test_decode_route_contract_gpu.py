"""csmoe_decode_route against its contract, point by point: the logits within the bound csmoe_gate_select is held to
(tests/test_ops_gpu.py::test_gate_select_equals_gate_then_select) against csmoe_gate_logits and the fp64 product; softmax / idx / w
the bits csmoe_router_select gives on ITS OWN logits, for all seven rules; the bins equal to csmoe_bin_tokens of a copy of idx (and
to the torch sort of tests/decode_route_ref.py); the quantised rows the bytes csmoe_quantize_mxfp8 writes.  Finite inputs only.
Shapes: the smallest that reach every path of the kernel -- one or several column blocks (E <= 16 or not) and row blocks (T <= 16 or
not: none, one or two in-launch hand-offs), fewer K-steps than waves, a ragged K-step, an uneven K split, every VPL of the selection
(E <= 64, <= 128, <= 256) and the limits E = 256 and T * K = 1024."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from competesmoe_amd import _lib as L
    from competesmoe_amd import ops

from tests.decode_route_ref import ref_bins

DEV = "cuda"
CASES = [(1, 128, 8, 2), (1, 4096, 64, 2), (1, 4096, 128, 2), (3, 64, 4, 4), (15, 136, 16, 1), (16, 128, 17, 2), (17, 1056, 64, 8),
         (33, 256, 65, 2), (40, 128, 200, 6), (64, 512, 256, 8), (128, 128, 64, 8), (512, 128, 8, 2)]
RULES = ["SEL_SOFTMAX", "SEL_RAW", "SEL_TOPK_SOFTMAX", "SEL_SIGMOID", "SEL_TOPK_SIGMOID", "SEL_TEMP_SOFTMAX_TOPK", "SEL_SIGMOID_NORM"]


def _param(mode):
    return 0.5 if mode in (L.SEL_TOPK_SIGMOID, L.SEL_TEMP_SOFTMAX_TOPK) else 1.0


@functools.lru_cache(maxsize=None)
def _inputs(T, D, E, K):
    """(x, w_gate, csmoe_gate_logits, fp64 product, csmoe_quantize_mxfp8 of a copy of x | None): computed once per shape, read only."""
    g = torch.Generator(device=DEV).manual_seed(T * 7 + E + D)
    x = torch.randn(T, D, device=DEV, generator=g).to(torch.bfloat16)
    wg = (torch.randn(E, D, device=DEV, generator=g) * D ** -0.5).to(torch.bfloat16)
    q = ops.quantize_mxfp8(x.clone()) if D % 32 == 0 else None
    return x, wg, ops.gate_logits(x, wg), x.double() @ wg.double().t(), q


def _check(T, D, E, K, mode, rs, x, wg, ref_logits, exact, q):
    want_quant = q is not None
    assert ops.decode_route_ok(x, wg, K, want_quant)
    logits, sm, idx, w, bins, xq, xs = ops.decode_route(x, wg, K, mode, bool(rs), param=_param(mode), want_quant=want_quant)
    # logits
    d = (logits.float() - ref_logits.float()).abs()
    print(f"T={T} D={D} E={E} K={K} mode={mode} rs={rs}: max |logits - gate_logits| {float(d.max()):.3e}, "
          f"against fp64 {float((logits.double() - exact).abs().max()):.3e}")
    assert (d <= 2.0 ** -7 * ref_logits.float().abs().clamp_min(2.0 ** -6)).all(), d.max()
    assert (logits.double() - exact).abs().max() <= 2.0 ** -7 * exact.abs().max().clamp_min(1.0)
    # selection: router_select's bits on these logits
    sm2, idx2, w2 = ops.router_select(logits, K, mode, bool(rs), param=_param(mode))
    assert torch.equal(idx, idx2) and torch.equal(w, w2) and torch.equal(sm, sm2)
    # bins: bin_tokens of a copy of idx, and the torch sort
    plain = ops.bin_tokens(idx.clone(), E)
    assert plain is not bins
    assert bins.n == T * K and bins.E == E and bins.K == K
    for a, b in ((bins.counts, plain.counts), (bins.offsets, plain.offsets), (bins.perm, plain.perm), (bins.slot_of, plain.slot_of)):
        assert torch.equal(a, b)
    for a, b in zip((bins.counts, bins.offsets, bins.perm, bins.slot_of), ref_bins(idx, E)):
        assert torch.equal(a.cpu(), b)
    # quantised rows
    if want_quant:
        assert xq.shape == (T, D) and xs.shape == (T, D // 32)
        assert torch.equal(xq, q[0]) and torch.equal(xs, q[1])
    else:
        assert xq is None and xs is None
    return logits, sm, idx, w, bins, xq, xs


@pytest.mark.parametrize("mode_name,rs", [("SEL_SOFTMAX", 1), ("SEL_TOPK_SOFTMAX", 1)])
@pytest.mark.parametrize("T,D,E,K", CASES)
def test_decode_route_contract(T, D, E, K, mode_name, rs):
    _check(T, D, E, K, getattr(L, mode_name), rs, *_inputs(T, D, E, K))


@pytest.mark.parametrize("rs", [0, 1])
@pytest.mark.parametrize("mode_name", RULES)
@pytest.mark.parametrize("T,D,E,K", [(17, 128, 8, 2), (40, 128, 200, 6)])
def test_decode_route_every_rule(T, D, E, K, mode_name, rs):
    _check(T, D, E, K, getattr(L, mode_name), rs, *_inputs(T, D, E, K))


@pytest.mark.parametrize("T,D,E,K", [(17, 128, 8, 2), (40, 128, 200, 6)])
def test_decode_route_ties_go_to_the_lower_index(T, D, E, K):
    """Gate rows duplicated in pairs: experts 2i and 2i + 1 have equal logits.  idx is still router_select's on these logits, and
    wherever the odd twin is selected the even one was selected before it."""
    x, wg, _, _, q = _inputs(T, D, E, K)
    wg = wg.clone()
    wg[1::2] = wg[0::2]
    logits, sm, idx, w, bins, xq, xs = _check(T, D, E, K, L.SEL_SOFTMAX, 1, x, wg, ops.gate_logits(x, wg), x.double() @ wg.double().t(), q)
    assert torch.equal(logits[:, 1::2], logits[:, 0::2])
    ids = idx.cpu().tolist()
    n_odd = 0
    for row in ids:
        for k, e in enumerate(row):
            if e % 2 == 1:
                n_odd += 1
                assert e - 1 in row[:k], row
    assert n_odd > 0


def _all_equal(a, b):
    for u, v in zip(a[:4] + a[5:], b[:4] + b[5:]):
        assert (u is None and v is None) or torch.equal(u, v)
    for u, v in zip((a[4].counts, a[4].offsets, a[4].perm, a[4].slot_of), (b[4].counts, b[4].offsets, b[4].perm, b[4].slot_of)):
        assert torch.equal(u, v)


def test_decode_route_repeated_calls_are_bit_identical():
    """(33, 256, 65, 2), then (1, 128, 8, 2), then the first again: a counter that is not zeroed again, a stale hand-off or an
    order-dependent sum would show as a difference between the two runs of the first shape."""
    big, small = (33, 256, 65, 2), (1, 128, 8, 2)
    first = _check(*big, L.SEL_SOFTMAX, 1, *_inputs(*big))
    _check(*small, L.SEL_SOFTMAX, 1, *_inputs(*small))
    again = _check(*big, L.SEL_SOFTMAX, 1, *_inputs(*big))
    _all_equal(first, again)


def test_decode_route_on_a_non_default_stream():
    case = (33, 256, 65, 2)
    inp = _inputs(*case)
    ref = _check(*case, L.SEL_TOPK_SOFTMAX, 1, *inp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = ops.decode_route(inp[0], inp[1], case[3], L.SEL_TOPK_SOFTMAX, True, want_quant=True)
    s.synchronize()
    _all_equal(ref, out)


def test_bin_tokens_and_quantize_pick_the_route_plan_up():
    T, D, E, K = 17, 128, 8, 2
    x, wg, _, _, q = _inputs(T, D, E, K)
    logits, sm, idx, w, bins, xq, xs = ops.decode_route(x, wg, K, L.SEL_SOFTMAX, True, want_quant=True)
    assert ops._route_plan_for(idx, E) is bins and ops.bin_tokens(idx, E) is bins
    assert ops.bin_tokens(idx.view(T * K).view(T, K), E) is bins
    got = ops.quantize_mxfp8(x)
    assert got[0] is xq and got[1] is xs
    ops.profile_start()
    copy = ops.bin_tokens(idx.clone(), E)                   # another tensor: the sort
    qc = ops.quantize_mxfp8(x.clone())
    prof = ops.profile_stop()
    assert copy is not bins and torch.equal(copy.perm, bins.perm) and torch.equal(copy.slot_of, bins.slot_of)
    assert prof.get("quantize_mxfp8", {}).get("calls", 0) == 1 and torch.equal(qc[0], xq) and torch.equal(qc[1], xs)
    idx[0, 0] = (idx[0, 0] + 1) % E                         # an in-place edit retires the bins
    assert ops._route_plan_for(idx, E) is None
    edited = ops.bin_tokens(idx, E)
    assert edited is not bins
    for a, b in zip((edited.counts, edited.offsets, edited.perm, edited.slot_of), ref_bins(idx, E)):
        assert torch.equal(a.cpu(), b)
    # the next routing call replaces the plan, a gate_select clears it
    out2 = ops.decode_route(x, wg, K, L.SEL_SOFTMAX, True)
    assert ops._route_plan_for(out2[2], E) is out2[4] and ops._quant_rows_for(x) is None
    ops.gate_select(x, wg, K, L.SEL_SOFTMAX, True)
    assert ops._ROUTE_PLAN is None
