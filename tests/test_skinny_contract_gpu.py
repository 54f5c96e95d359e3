"""csmoe_grouped_gemm_skinny (csrc/gemm_skinny.hip) held to the epilogue contract of include/csmoe.h on the exact data of
tests/gemm_contract.py, bit for bit where the contract fixes the bits, and to the tiled kernels' own results on the same data.

Shapes: expert row counts [0, 1, 16, 17, 3, 0, 33] (an empty expert first and in the middle, one row, exactly one 16-row block, a
block plus one, two blocks plus one; M = 70), N in {72, 200} (neither a multiple of 16; 200 crosses the widest column slab, 64),
Kd in {40, 1096} (one whole K-step + a partial one; many K-steps split over the 8 waves + a partial last one).  Kd <= 2048, so the
exactness argument of gemm_contract holds for any summation order, the kernel's split of K over its waves included.

Out-of-bounds stores: C / C2 live inside a buffer of M + 16 rows with ldc = N + 24 pre-filled with a sentinel, and every element
outside [0, M) x [0, N) must still hold it.  Out-of-bounds loads are not provoked: A has exactly M rows (or exactly the source rows
of the gather), and the kernel's header comment argues from its address arithmetic that no other row is read.
"""
import functools

import pytest
import torch

from tests import gemm_contract as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from competesmoe_amd import ops, _lib as L

DEV = "cuda"
BF = torch.bfloat16
COUNTS = [0, 1, 16, 17, 3, 0, 33]
E, M = len(COUNTS), sum(COUNTS)
SENTINEL = -12288.0                     # bf16-exact, never produced by the data
SHAPES = [(layout, N, Kd) for layout in (0, 1) for N in (72, 200) for Kd in (40, 1096)]
RTOL, ATOL = 2.0 ** -7, 2e-2            # the bound tests/test_gemm_fuzz_gpu.py holds the bf16 kernels to


def _offsets():
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = torch.tensor(COUNTS).cumsum(0)
    return off


def _expert_rows(off):
    return torch.repeat_interleave(torch.arange(E), (off[1:] - off[:-1]).long())


class Case:
    """Exact operands of one (layout, N, Kd), their fp64 accumulator, and device copies.  Built once and never modified."""

    def __init__(self, layout, N, Kd):
        g = torch.Generator().manual_seed(1000 * layout + 10 * N + Kd)
        self.layout, self.N, self.Kd = layout, N, Kd
        self.off = _offsets()
        self.A = G.rows_a(M, Kd, g)
        shape = (N, Kd) if layout == 0 else (Kd, N)
        self.B = [G.weights_b(shape, g) for _ in range(E)]
        bias = [G.bias_bf16(N, g) for _ in range(E)]
        bias32 = [G.bias_f32(N, g) for _ in range(E)]
        er = _expert_rows(self.off)
        self.acc = torch.zeros(M, N, dtype=torch.float64)
        for e in range(E):
            r0, r1 = int(self.off[e]), int(self.off[e + 1])
            if r1 > r0:
                self.acc[r0:r1] = self.A[r0:r1].double() @ (self.B[e].double().t() if layout == 0 else self.B[e].double())
        self.bias_rows = torch.stack(bias)[er].float()
        self.bias32_rows = torch.stack(bias32)[er]
        self.ldb = Kd if layout == 0 else N
        self.dA = self.A.to(BF).to(DEV)                        # exactly M rows
        self.dB = [b.to(BF).to(DEV) for b in self.B]
        self.dBp = ops.ptr_array(self.dB, DEV)
        self.dbias = [b.to(DEV) for b in bias]
        self.dbiasp = ops.ptr_array(self.dbias, DEV)
        self.dbias32 = [b.to(DEV) for b in bias32]
        self.dbias32p = ops.ptr_array(self.dbias32, DEV)
        self.doff = self.off.to(DEV)

    def bias_ptrs(self, epi):
        return self.dbiasp if epi in (G.BIAS, G.BIAS_ACT) else self.dbias32p if epi == G.R32_ACT else None

    def ref(self, epi, act):
        kw = {}
        if epi in (G.BIAS, G.BIAS_ACT):
            kw["bias"] = self.bias_rows
        if epi == G.R32_ACT:
            kw["bias"] = self.bias32_rows
        return G.epilogue_ref(self.acc, epi, act, dtype=BF, **kw)


@functools.lru_cache(maxsize=None)
def _case(layout, N, Kd):
    return Case(layout, N, Kd)


def _launches():
    out = [(G.PLAIN, G.NONE, True), (G.BIAS, G.NONE, True)]
    for epi in (G.BIAS_ACT, G.R32_ACT):
        for act in G.ACTS:
            out += [(epi, act, True), (epi, act, False)]
    return out


def _skinny(c, epi, act, want_c, A=None, src_rows=None, src_div=1):
    """One launch into sentinel-filled buffers of M + 16 rows, ldc = N + 24; returns the (C, C2) buffers (None where not asked)."""
    has_c2 = epi in (G.BIAS_ACT, G.R32_ACT)
    bufs = [torch.full((M + 16, c.N + 24), SENTINEL, dtype=BF, device=DEV) if w else None for w in (want_c, has_c2)]
    views = [None if b is None else b[:M, :c.N] for b in bufs]
    ops.grouped_gemm_skinny(c.dA if A is None else A, c.dBp, c.layout, c.ldb, c.N, c.doff, E, bias_ptrs=c.bias_ptrs(epi),
                            epilogue=epi, act=act, want_c=want_c, want_c2=has_c2, src_rows=src_rows, src_div=src_div,
                            out=views[0], out2=views[1])
    return bufs


def _check_sentinel(buf, N, what):
    b = buf.cpu().float()
    assert bool((b[M:] == SENTINEL).all()), f"{what}: rows past M written"
    assert bool((b[:M, N:] == SENTINEL).all()), f"{what}: columns past N written"


@pytest.mark.parametrize("layout,N,Kd", SHAPES)
def test_skinny_contract(layout, N, Kd):
    c = _case(layout, N, Kd)
    if Kd == 1096:
        assert G.count_ties(c.acc) > 0                     # the bf16 rounding of the accumulator is exercised on exact ties
    for epi, act, want_c in _launches():
        what = f"skinny layout={layout} N={N} Kd={Kd} {G.EPI_NAMES[epi]} {G.ACT_NAMES[act]} C={want_c}"
        ref = c.ref(epi, act)
        bufs = _skinny(c, epi, act, want_c)
        has_c2 = epi in (G.BIAS_ACT, G.R32_ACT)
        # the tiled kernel the library picks for this launch today, on the same data
        tiled = ops.grouped_gemm(c.dA, c.dBp, layout, c.ldb, N, c.doff, E, bias_ptrs=c.bias_ptrs(epi), epilogue=epi, act=act,
                                 want_c2=has_c2, want_c=want_c, kernel=0)
        tiled = tiled if has_c2 else (tiled, None)
        for name, buf, other in zip(("C", "C2"), bufs, tiled):
            if buf is None:
                continue
            _check_sentinel(buf, N, what + " " + name)
            got = buf[:M, :N]
            G.compare(got, ref[name], G.is_exact(epi, act, name), gelu=act in G.GELU_FAMILY, g=ref.get("g"), dtype=BF,
                      what=what + " " + name)
            assert torch.equal(got.contiguous().view(torch.int16), other.view(torch.int16)), what + f" {name}: differs from kernel=0"


@pytest.mark.parametrize("layout,N,Kd", SHAPES)
def test_skinny_gather(layout, N, Kd):
    """src_rows = a permutation of the 70 flat (token, k) slots of 35 source rows with src_div = 2: every source row is read twice,
    as K = 2 routing does; equal to the ungathered launch on the materialised rows."""
    c = _case(layout, N, Kd)
    g = torch.Generator().manual_seed(7)
    src = G.rows_a(M // 2, Kd, g).to(BF)                       # exactly the 35 source rows
    perm = torch.randperm(M, generator=g).int()
    dsrc, dperm = src.to(DEV), perm.to(DEV)
    rows = dsrc[(dperm // 2).long()].contiguous()
    for epi, act in ((G.PLAIN, G.NONE), (G.BIAS_ACT, G.GELU)):
        gathered = _skinny(c, epi, act, True, A=dsrc, src_rows=dperm, src_div=2)
        plain = _skinny(c, epi, act, True, A=rows)
        for name, a, b in zip(("C", "C2"), gathered, plain):
            if a is not None:
                _check_sentinel(a, N, f"gather {name}")
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"gather layout={layout} N={N} Kd={Kd} {name}"


@pytest.mark.parametrize("layout,N,Kd", SHAPES)
def test_skinny_random_and_deterministic(layout, N, Kd):
    """randn rows, randn / sqrt(Kd) weights against the fp64 product rounded once; a second run of the same launch is bit-identical
    (K is split over the waves of a workgroup and summed in a fixed order)."""
    g = torch.Generator().manual_seed(11 + layout)
    off = _offsets()
    A = torch.randn(M, Kd, generator=g).to(BF)
    B = [(torch.randn((N, Kd) if layout == 0 else (Kd, N), generator=g) / Kd ** 0.5).to(BF) for _ in range(E)]
    ref = torch.zeros(M, N, dtype=torch.float64)
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            ref[r0:r1] = A[r0:r1].double() @ (B[e].double().t() if layout == 0 else B[e].double())
    ref = ref.float().to(BF).float()
    dB = [b.to(DEV) for b in B]
    run = lambda: ops.grouped_gemm_skinny(A.to(DEV), ops.ptr_array(dB, DEV), layout, Kd if layout == 0 else N, N, off.to(DEV), E)
    c1, c2 = run(), run()
    assert torch.equal(c1.view(torch.int16), c2.view(torch.int16))
    torch.testing.assert_close(c1.float().cpu(), ref, rtol=RTOL, atol=ATOL)
