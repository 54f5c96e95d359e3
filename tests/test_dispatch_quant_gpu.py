"""GPU: csmoe_dispatch_rows_mxfp8 / csmoe_dispatch_tokens_mxfp8 (gather rows into the binned row space and quantise them in one pass)
write, byte for byte, what ops.dispatch_rows / ops.dispatch_tokens followed by ops.quantize_mxfp8 write, and what oracle.mxfp8.quantize
gives for the gathered rows.  Every comparison is torch.equal.  (Where a block holds a NaN the project's quantisers skip it in the
block's amax and keep it a NaN -- tests/test_fp8_gpu.py::test_quantisers_keep_a_nan_and_saturate_an_inf; the oracle is given the row
with the NaN removed and the NaN bytes are checked apart, as there.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


@pytest.fixture(autouse=True)
def _fused_on(monkeypatch):
    from competesmoe_amd import ops
    monkeypatch.setattr(ops, "_DISPATCH_QUANT", True)          # the one-pass kernels, whatever CSMOE_DISPATCH_QUANT says


def _routing(kind, T, K, E, g):
    if kind == "random":
        return torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(T)]).int()
    if kind == "empty":                     # only the odd experts of the upper half are ever chosen: most experts hold nothing
        pool = torch.arange(E // 2 + 1, E, 2) if E >= 4 * K else torch.arange(E - K, E)
        return torch.stack([pool[torch.randperm(pool.numel(), generator=g)[:K]] for _ in range(T)]).int()
    if kind == "one":                       # slot 0 of every token goes to expert 1
        idx = torch.stack([(torch.randperm(E - 2, generator=g)[:K] + 2) for _ in range(T)]).int()
        idx[:, 0] = 1
        return idx
    raise ValueError(kind)


def _special_rows(x):
    """Rows 0..5 of x: zeros, a NaN, saturation-edge values 448 * 2^k and just above, bf16 subnormals, mixed huge / tiny blocks."""
    T, D = x.shape
    x[0] = 0
    x[1, D // 2 + 3] = float("nan")
    k = torch.arange(D) % 24 - 12
    x[2] = (448.0 * torch.pow(2.0, k.float())).bfloat16() * torch.where(torch.arange(D) % 3 == 0, -1.0, 1.0).bfloat16()
    edge = torch.tensor([448.0, 464.0, 480.0, 496.0, 446.0, 432.0, 256.0, 400.0])     # block amax 496: above 448 at scale 1
    x[3] = (edge[torch.arange(D) % 8] * torch.pow(2.0, ((torch.arange(D) // 32) % 9 - 4).float())).bfloat16()
    sub = ((torch.arange(D) % 127) + 1).to(torch.int16)                      # bf16 bit patterns 0x0001 .. 0x007f: subnormals
    sub = torch.where(torch.arange(D) % 5 == 0, sub | torch.tensor(-32768, dtype=torch.int16), sub)     # some negative
    x[4] = sub.view(torch.bfloat16)
    x[5] = x[5] * torch.where(torch.arange(D) % 64 < 32, 3.0e38, 1.0e-30).bfloat16()
    return x


def _check(x, idx, E, oracle_rows=None):
    from competesmoe_amd import ops
    from oracle import mxfp8 as MX
    T, D = x.shape
    xg, ig = x.to(DEV), idx.to(DEV)
    bins = ops.bin_tokens(ig, E)
    ref_xs = ops.dispatch_tokens(xg, bins)
    assert torch.equal(ops.dispatch_rows(xg, bins).view(torch.int16), ref_xs.view(torch.int16))
    ref_q, ref_s = ops.quantize_mxfp8(ref_xs)
    for fn in (ops.dispatch_tokens_mxfp8, ops.dispatch_rows_mxfp8):
        for want_rows in (True, False):
            xs, q, s = fn(xg, bins, want_rows=want_rows)
            if want_rows:
                assert torch.equal(xs.view(torch.int16), ref_xs.view(torch.int16)), (fn.__name__, "rows")      # bits: NaN == NaN
            else:
                assert xs is None
            assert q.shape == (bins.n, D) and s.shape == (bins.n, D // 32) and q.dtype == s.dtype == torch.uint8
            assert torch.equal(q, ref_q), (fn.__name__, want_rows, "elements")
            assert torch.equal(s, ref_s), (fn.__name__, want_rows, "scales")
    # the oracle on the gathered rows (bins.perm[m] // K is row m's token)
    n = bins.n if oracle_rows is None else min(bins.n, oracle_rows)
    src = (bins.perm[:n].long() // bins.K).cpu()
    rows = x[src].float()
    nan_at = torch.isnan(rows)
    oq, os_ = MX.quantize(torch.where(nan_at, torch.zeros_like(rows), rows))          # +-Inf stays (nan_to_num would make it finite)
    q, s = ref_q[:n].cpu(), ref_s[:n].cpu()
    xs, fq, fs = ops.dispatch_rows_mxfp8(xg, bins)
    fq, fs = fq[:n].cpu(), fs[:n].cpu()
    assert torch.equal(fs, os_) and torch.equal(fq[~nan_at], oq[~nan_at])
    assert bool(((fq[nan_at] & 0x7F) == 0x7F).all()), "a NaN was turned into a finite e4m3 value"
    assert torch.equal(q, fq) and torch.equal(s, fs)


@pytest.mark.parametrize("D", [32, 64, 4096, 4128])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_one_pass_dispatch_quantise_is_the_two_launches_byte_for_byte(D, K):
    g = torch.Generator().manual_seed(100 * K + D)
    T, E = 203, 16
    x = _special_rows(torch.randn(T, D, generator=g).bfloat16())
    _check(x, _routing("random", T, K, E, g), E)


@pytest.mark.parametrize("kind", ["empty", "one"])
@pytest.mark.parametrize("K,D", [(1, 64), (2, 4128), (8, 4096)])
def test_routings_with_empty_experts_and_one_expert_taking_everything(kind, K, D):
    g = torch.Generator().manual_seed(7 * K + D)
    T, E = 150, 32
    x = _special_rows(torch.randn(T, D, generator=g).bfloat16())
    idx = _routing(kind, T, K, E, g)
    _check(x, idx, E)
    if kind == "one" and K == 1:
        assert int((idx == 1).sum()) == T


def test_regroup_permutation_of_an_expert_parallel_lane():
    """The K = 1 regroup of rows received from several peers (ep._Lane.arrived_mxfp8): a permutation gather."""
    from competesmoe_amd import ops
    g = torch.Generator().manual_seed(3)
    n, D, E = 777, 256, 5
    x = _special_rows(torch.randn(n, D, generator=g).bfloat16()).to(DEV)
    ids = torch.randint(0, E, (n, 1), generator=g).int().to(DEV)
    lb = ops.bin_tokens(ids, E)
    rs, q, s = ops.dispatch_rows_mxfp8(x, lb)
    ref = ops.dispatch_rows(x, lb)
    rq, rsc = ops.quantize_mxfp8(ref)
    assert torch.equal(rs.view(torch.int16), ref.view(torch.int16)) and torch.equal(q, rq) and torch.equal(s, rsc)


def test_switch_off_takes_the_two_launches(monkeypatch):
    from competesmoe_amd import ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(64, 128, generator=g).bfloat16().to(DEV)
    bins = ops.bin_tokens(_routing("random", 64, 2, 8, g).to(DEV), 8)
    on = ops.dispatch_tokens_mxfp8(x, bins)
    monkeypatch.setattr(ops, "_DISPATCH_QUANT", False)
    called = []
    real = ops.quantize_mxfp8
    monkeypatch.setattr(ops, "quantize_mxfp8", lambda t, transpose=False: (called.append(1), real(t, transpose))[1])
    off = ops.dispatch_tokens_mxfp8(x, bins)
    assert called and all(torch.equal(a, b) for a, b in zip(on, off))
    assert ops.dispatch_rows_mxfp8(x, bins, want_rows=False)[0] is None


def test_wrappers_refuse_what_the_kernel_cannot_take():
    from competesmoe_amd import ops
    x = torch.randn(16, 48).bfloat16().to(DEV)
    bins = ops.bin_tokens(torch.zeros(16, 1, dtype=torch.int32, device=DEV), 2)
    with pytest.raises(ValueError, match="D % 32"):
        ops.dispatch_tokens_mxfp8(x, bins)
    with pytest.raises(ValueError):
        ops.dispatch_rows_mxfp8(torch.randn(16, 64, device=DEV), bins)         # fp32 rows


def test_headline_size_once():
    """T = 32 768, D = 4096, K = 2 (BASELINE config 5's token side); the oracle on the first 512 binned rows, the two-launch path on
    all of them."""
    g = torch.Generator().manual_seed(9)
    T, D, K, E = 32768, 4096, 2, 128
    x = torch.randn(T, D, generator=g).bfloat16()
    first = torch.randint(0, E, (T,), generator=g)
    idx = torch.stack([first, (first + 1 + torch.randint(0, E - 1, (T,), generator=g)) % E], 1).int()
    _check(x, idx, E, oracle_rows=512)
