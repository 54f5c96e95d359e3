"""GPU: every GEMM kernel against the epilogue contract of include/csmoe.h, bit for bit on exact data (tests/gemm_contract.py).

The reference, the data and the exactness argument are in tests/gemm_contract.py: on that data the fp32 accumulator is exact in any
summation order, so every difference left is an epilogue difference.  Each test loops over the epilogues and activations on shared
operands; a failure names the epilogue, the activation and the first bad element.

Coverage (kernel x epilogue x activation x layout; acts = NONE, ReLU, GELU, GELU_TANH, SiLU, quick-GELU):

  kernel (how it is reached)                    layouts   epilogues                                           test
  gg_generic_kernel fp32 (fp32 operands)        NK, KN    PLAIN, BIAS(+/-bias), BIAS_ACT x acts, R32 x acts,   test_grouped_contract[generic32-*]
                                                          ACTGRAD x acts, ROWSCALE x acts (no dot table)
  gg_generic_kernel bf16 (force_generic)        NK, KN    same; a dot table is refused                        test_grouped_contract[generic16-*]
  gg_fast_kernel 128x128 (kernel=0, M < 2048)   NK, KN    same + ROWSCALE dot table [M][N/8]                  test_grouped_contract[fast128-*]
  gg8_kernel BAL (NK) / WIDE (KN), thin loop    NK, KN    same + dot table [M][ceil(N/128)]                   test_grouped_contract[gg8-*]
  gg4_kernel, its three K-loop forms            NK        same                                                test_grouped_contract[gg4-nk]
  gg8c_kernel + gg8_rowspace_rest (f32w)        KN        PLAIN..R32 x acts, with / without the bf16 copy     test_f32w_contract[*]
  dense entry (single_B / single_bias)          NK, KN    PLAIN, BIAS, BIAS_ACT, R32, ACTGRAD x acts, ACCUM;  test_dense_contract[*]
    on generic bf16, 128-tile, gg8, gg4                   SOFTPLUS_ROWSUM / _GRAD (flags 0..3) on gg8 / gg4
  the tiled bf16 kernels against each other     NK, KN    every epilogue x act: bit-identical                 test_tiled_kernels_agree
  gg8_kernel WIDE on NK / BAL on KN, no thin    NK, KN    process switches in fresh children (CSMOE_GEMM_SCHED=2 / 3, CSMOE_THIN_LOOP=0,
    loop, f32w unsplit, 128-tile at a big                 CSMOE_F32W_SPLIT=0, CSMOE_GEMM_KERNEL=v1, CSMOE_GEMM_PERSISTENT=0)
    shape, gg8w one workgroup per tile                    against the default run and the reference           test_process_switches[*]
  weight gradients: generic, 128-tile, gg8w     -         fp32 / bf16 out, accumulate on / off, contiguous /  test_wgrad_contract[*],
    (grouped and dense), split-K pseudo-experts           dealt experts, canaries in [Nb, ldc), empty experts  test_dense_wgrad_contract
  every kernel, random data, Kd 1k..4k          NK, KN    PLAIN, fp64 bound of test_guards_gpu                test_random_data_bound[*]
  dot table vs kernel selector (kernel=2 / 4, M < 2048): refused before launching                            test_rowdot_kernel_selector
  hipFuncSetAttribute per instantiation (common.h set_dyn_lds): ACCUM first on gg8 / gg4, then the others, in a fresh child   test_lds_attribute_per_instantiation

Edges: expert rows 0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 256k + {64, 65, 192, 193}, an empty expert first and last; N a
multiple of 8 but not of 128 (136, 264, 520); Kd a multiple of 8 but not of 64 (200, 520) except on gg4; lda > Kd (A's extra columns hold
NaN), ldc > N; C, C2, aux and the dot table live in larger buffers whose rows [offsets[E], M) and columns [N, ldc) hold a canary that
must come back bit-identical; M = 0 writes nothing.

Observed figures (ulp / mismatch per comparison class) are recorded in tests/gemm_contract.py's docstring.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import gemm_contract as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from competesmoe_amd import ops, _lib as L
    from tests.test_guards_gpu import gemm_bound_ok

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = -12288.0                       # bf16- and fp32-exact, never produced by the data

# row counts of the experts (first and last empty)
ROWS_SMALL = [0, 1, 15, 17, 64, 65, 129, 0]
ROWS_128 = [0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 0]                               # 1201 rows: M < 2048
ROWS_256 = [0, 1, 17, 128, 129, 255, 256, 257, 256 + 64, 256 + 65, 256 + 192, 256 + 193, 0]  # 2581 rows: M >= 2048


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offsets(counts):
    off = torch.zeros(len(counts) + 1, dtype=torch.int32)
    off[1:] = torch.tensor(counts).cumsum(0)
    return off


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _expert_rows(off):
    """[M_used] expert index of every binned row."""
    counts = (off[1:] - off[:-1]).long()
    return torch.repeat_interleave(torch.arange(len(counts)), counts)


class Operands:
    """Exact operands of one grouped launch family, in padded buffers (lda > Kd, ldc > N) with canaries."""

    def __init__(self, counts, N, Kd, layout, dtype, seed, pad_rows=3):
        g = torch.Generator().manual_seed(seed)
        self.E, self.N, self.Kd, self.layout, self.dtype = len(counts), N, Kd, layout, dtype
        self.off = _offsets(counts)
        self.used = int(self.off[-1])
        self.M = self.used + pad_rows
        self.lda, self.ldc = Kd + 8, N + 8
        a = G.rows_a(self.M, Kd, g)
        self.A_buf = torch.full((self.M, self.lda), float("nan"), dtype=dtype)
        self.A_buf[:self.used, :Kd] = a[:self.used]
        self.A = a[:self.used]
        shape = (N, Kd) if layout == 0 else (Kd, N)
        self.B = [G.weights_b(shape, g) for _ in range(self.E)]
        self.bias = [G.bias_bf16(N, g) for _ in range(self.E)]
        self.bias32 = [G.bias_f32(N, g) for _ in range(self.E)]
        self.aux = G.aux_grid((self.M, N), g)
        self.scale = G.row_scales(self.M, g)
        er = _expert_rows(self.off)
        # exact accumulator per binned row (fp64)
        acc = torch.zeros(self.used, N, dtype=torch.float64)
        for e in range(self.E):
            r0, r1 = int(self.off[e]), int(self.off[e + 1])
            if r1 > r0:
                Bt = self.B[e].double().t() if layout == 0 else self.B[e].double()
                acc[r0:r1] = self.A[r0:r1].double() @ Bt
        self.acc = acc
        self.bias_rows = torch.stack(self.bias)[er].float() if self.used else torch.zeros(0, N)
        self.bias32_rows = torch.stack(self.bias32)[er] if self.used else torch.zeros(0, N)
        # device copies
        self.dA = self.A_buf.to(DEV)
        self.dB = [b.to(dtype).to(DEV) for b in self.B]
        self.dBp = ops.ptr_array(self.dB, DEV)
        bdt = dtype                                  # BIAS / BIAS_ACT read the bias in the operand dtype
        self.dbias = [b.to(bdt).to(DEV) for b in self.bias]
        self.dbiasp = ops.ptr_array(self.dbias, DEV)
        self.dbias32 = [b.to(DEV) for b in self.bias32]
        self.dbias32p = ops.ptr_array(self.dbias32, DEV)
        self.doff = self.off.to(DEV)
        aux_buf = torch.full((self.M, self.ldc), float("nan"), dtype=dtype)
        aux_buf[:, :N] = self.aux.to(dtype)
        self.daux = aux_buf.to(DEV)
        self.dscale = self.scale.to(DEV)

    def out_buf(self):
        return torch.full((self.M, self.ldc), CANARY, dtype=self.dtype, device=DEV)

    def check_canary(self, buf, what):
        """Rows [offsets[E], M) and columns [N, ldc) must hold the canary, bit for bit."""
        want = torch.full((), CANARY, dtype=buf.dtype)
        b = buf.cpu()
        tail = b[self.used:]
        side = b[:self.used, self.N:]
        for name, part in (("rows past offsets[E]", tail), ("columns past N", side)):
            if part.numel() and not torch.equal(_bits(part), _bits(want.expand_as(part).contiguous())):
                bad = (_bits(part) != _bits(want.expand_as(part).contiguous())).nonzero()[0].tolist()
                raise AssertionError(f"{what}: {name} overwritten at {bad}")


def grouped(o: Operands, epi, act, kernel, *, bias="bf16", want_c=True, want_c2=None, dot=None):
    """One csmoe_grouped_gemm launch on o's buffers; returns (rc, C_buf, C2_buf)."""
    if want_c2 is None:
        want_c2 = epi in (G.BIAS_ACT, G.R32_ACT)
    C = o.out_buf() if want_c else None
    C2 = o.out_buf() if want_c2 else None
    bp = None
    if epi in (G.BIAS, G.BIAS_ACT) and bias is not None:
        bp = o.dbiasp
    if epi == G.R32_ACT and bias is not None:
        bp = o.dbias32p
    c2p = C2
    if epi == G.ROWSCALE:
        c2p = o.dscale
        if dot is not None:
            bp = ops.ptr_table(dot, o.E, 0)
    aux = o.daux if epi in (G.ACTGRAD, G.ROWSCALE) else None
    dt = L.BF16 if o.dtype == BF else L.F32
    rc = L.lib.csmoe_grouped_gemm(o.dA.data_ptr(), o.lda, o.dBp.data_ptr(), o.layout, o.Kd if o.layout == 0 else o.N,
                                  None if bp is None else bp.data_ptr(), o.doff.data_ptr(), o.E, o.M, o.N, o.Kd,
                                  None if C is None else C.data_ptr(), None if c2p is None else c2p.data_ptr(),
                                  None if aux is None else aux.data_ptr(), o.ldc, epi, act, dt, kernel, _stream())
    return rc, C, C2


def _ref(o: Operands, epi, act, bias="bf16"):
    kw = {}
    if epi in (G.BIAS, G.BIAS_ACT) and bias is not None:
        kw["bias"] = o.bias_rows
    if epi == G.R32_ACT and bias is not None:
        kw["bias"] = o.bias32_rows
    if epi in (G.ACTGRAD, G.ROWSCALE):
        kw["aux"] = o.aux[:o.used].to(o.dtype)
    if epi == G.ROWSCALE:
        kw["scale"] = o.scale[:o.used]
    return G.epilogue_ref(o.acc, epi, act, dtype=o.dtype, **kw)


STATS = {}


def _check_out(o, buf, ref, epi, act, out, what):
    n = o.N
    got = buf[:o.used, :n]
    exact = G.is_exact(epi, act, out)
    ulps, frac = G.compare(got, ref[out], exact, gelu=act in G.GELU_FAMILY, g=ref.get("g"), dtype=o.dtype, what=what)
    if not exact:
        k = (o.dtype, G.ACT_NAMES[act])
        u0, f0 = STATS.get(k, (0.0, 0.0))
        STATS[k] = (max(u0, ulps), max(f0, frac))
    o.check_canary(buf, what)


def _cases(tiled):
    """(epilogue, act, options) of one loop: every epilogue the grouped entry accepts, every act where it has one, null forms."""
    out = [(G.PLAIN, G.NONE, {}), (G.BIAS, G.NONE, {}), (G.BIAS, G.NONE, {"bias": None})]
    for act in G.ACTS:
        out += [(G.BIAS_ACT, act, {}), (G.R32_ACT, act, {}), (G.ACTGRAD, act, {}), (G.ROWSCALE, act, {"dot": tiled and act in (G.RELU, G.GELU)})]
    out += [(G.BIAS_ACT, G.GELU, {"bias": None}), (G.BIAS_ACT, G.RELU, {"want_c": False}), (G.R32_ACT, G.SILU, {"want_c": False}),
            (G.R32_ACT, G.QUICK_GELU, {"bias": None})]
    return out


def run_contract(o: Operands, kernel, dot_cols, tag):
    """Every case of _cases on one operand family; dot_cols = the dot table's columns (0: the launch must refuse a table)."""
    ties = G.count_ties(o.acc)
    assert ties > 20, f"{tag}: only {ties} rounding ties in the accumulator: the data no longer tests round-to-nearest-even"
    for epi, act, opt in _cases(dot_cols > 0):
        what = f"{tag} {G.EPI_NAMES[epi]} act={G.ACT_NAMES[act]} {opt}"
        dot = None
        if opt.get("dot"):
            dot = torch.full((o.M + 2, dot_cols), CANARY, dtype=F32, device=DEV)
        kw = {k: v for k, v in opt.items() if k != "dot"}
        rc, C, C2 = grouped(o, epi, act, kernel, dot=dot, **kw)
        torch.cuda.synchronize()
        assert rc == 0, f"{what}: rc {rc}: {L.lib.csmoe_last_error().decode()}"
        ref = _ref(o, epi, act, bias=kw.get("bias", "bf16"))
        if C is not None:
            _check_out(o, C, ref, epi, act, "C", what + " C")
        if C2 is not None:
            _check_out(o, C2, ref, epi, act, "C2", what + " C2")
        if dot is not None:
            d = dot.cpu()
            assert torch.equal(_bits(d[o.used:]), _bits(torch.full_like(d[o.used:], CANARY))), f"{what}: dot table rows past offsets[E] written"
            G.check_fp32_sums(d[:o.used].double().sum(1), ref["dot_terms"], what + " dot table")
    if dot_cols == 0 and o.dtype == BF:
        dot = torch.full((o.M, 64), CANARY, dtype=F32, device=DEV)
        rc, C, _ = grouped(o, G.ROWSCALE, G.RELU, kernel, dot=dot)
        torch.cuda.synchronize()
        assert rc == 3, f"{tag}: the generic kernel took a dot table (rc {rc})"
        assert bool((C.cpu() == CANARY).all()) and bool((dot.cpu() == CANARY).all()), f"{tag}: a refused launch wrote"


GROUPED = {
    # name: (counts, N, Kd, layout, dtype, kernel, expected rowdot_cols (None: not a bf16 fast shape))
    "generic32-nk": (ROWS_SMALL, 136, 520, 0, F32, 0, 0),
    "generic32-kn": (ROWS_SMALL, 136, 520, 1, F32, 0, 0),
    "generic16-nk": (ROWS_SMALL, 136, 520, 0, BF, 1, 0),
    "generic16-kn": (ROWS_SMALL, 136, 520, 1, BF, 1, 0),
    "fast128-nk": (ROWS_128, 264, 200, 0, BF, 0, 264 // 8),
    "fast128-kn": (ROWS_128, 264, 200, 1, BF, 0, 264 // 8),
    "gg8-nk": (ROWS_256, 264, 200, 0, BF, 2, 3),
    "gg8-kn": (ROWS_256, 264, 200, 1, BF, 2, 3),
    "gg4-nk": (ROWS_256, 520, 256, 0, BF, 4, 5),
}


@pytest.mark.parametrize("name", list(GROUPED))
def test_grouped_contract(name):
    counts, N, Kd, layout, dtype, kernel, dot_cols = GROUPED[name]
    o = Operands(counts, N, Kd, layout, dtype, seed=list(GROUPED).index(name))
    # pin the kernel family where the host can see it: 0 = generic, N/8 = 128-tile, ceil(N/128) = 256-tile
    rd = ops.rowdot_cols(o.M, N, Kd, o.lda, Kd if layout == 0 else N, o.ldc, dtype)
    if dtype == F32:
        assert rd == 0
    elif kernel != 1:
        assert rd == dot_cols, (name, rd)
    run_contract(o, kernel, dot_cols if kernel != 1 else 0, name)
    print(f"{name}: transcendental (max ulp, mismatch fraction) so far {STATS}")
    # M = 0: nothing written
    C = o.out_buf()
    rc = L.lib.csmoe_grouped_gemm(o.dA.data_ptr(), o.lda, o.dBp.data_ptr(), layout, Kd if layout == 0 else N, None,
                                  torch.zeros(o.E + 1, dtype=torch.int32, device=DEV).data_ptr(), o.E, 0, N, Kd, C.data_ptr(), None,
                                  None, o.ldc, G.PLAIN, 0, L.BF16 if dtype == BF else L.F32, kernel, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((C.cpu() == CANARY).all()), f"{name}: M = 0 wrote"


# ------------------------------------------------------------------------------------------------ fp32 masters (gg8c + rest)
@pytest.mark.parametrize("with_copy", [False, True])
def test_f32w_contract(with_copy):
    o = Operands(ROWS_256, 264, 200, 1, BF, seed=7)
    # fp32 masters just below the bf16 grid value (toward zero): round-to-nearest-even gives the grid back, truncation would not
    B32 = torch.stack([b - torch.sign(b) * b.abs() * 2.0 ** -12 for b in o.B]).to(DEV)
    copy = torch.full((o.E, o.Kd, o.N), CANARY, dtype=BF, device=DEV) if with_copy else None
    cp = ops.ptr_table(copy, o.E, o.Kd * o.N * 2) if with_copy else None
    bp = ops.ptr_table(B32, o.E, o.Kd * o.N * 4)
    for epi, act, opt in _cases(False):
        if epi == G.ROWSCALE:
            continue                                      # csmoe_grouped_gemm_f32w takes epilogues 0..4
        what = f"f32w copy={with_copy} {G.EPI_NAMES[epi]} act={G.ACT_NAMES[act]} {opt}"
        want_c = opt.get("want_c", True)
        want_c2 = epi in (G.BIAS_ACT, G.R32_ACT)
        C = o.out_buf() if want_c else None
        C2 = o.out_buf() if want_c2 else None
        b = opt.get("bias", "bf16")
        bias = None if b is None else (o.dbiasp if epi in (G.BIAS, G.BIAS_ACT) else o.dbias32p if epi == G.R32_ACT else None)
        rc = L.lib.csmoe_grouped_gemm_f32w(o.dA.data_ptr(), o.lda, bp.data_ptr(), o.N, None if cp is None else cp.data_ptr(),
                                           None if bias is None else bias.data_ptr(), o.doff.data_ptr(), o.E, o.M, o.N, o.Kd,
                                           None if C is None else C.data_ptr(), None if C2 is None else C2.data_ptr(),
                                           o.daux.data_ptr() if epi == G.ACTGRAD else None, o.ldc, epi, act, _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{what}: {L.lib.csmoe_last_error().decode()}"
        ref = _ref(o, epi, act, bias=b)
        if C is not None:
            _check_out(o, C, ref, epi, act, "C", what + " C")
        if C2 is not None:
            _check_out(o, C2, ref, epi, act, "C2", what + " C2")
    if with_copy:
        cpy = copy.cpu()
        for e in range(o.E):
            if int(o.off[e + 1]) > int(o.off[e]):
                assert torch.equal(cpy[e].float(), o.B[e]), f"bf16 copy of expert {e}"
            else:
                assert bool((cpy[e] == CANARY).all()), f"copy of empty expert {e} written"


# ------------------------------------------------------------------------------------------------ dense entry
DENSE = {
    # name: (M, N, Kd, layout, kernel, force_generic)
    "generic16-nk": (300, 136, 520, 0, 0, True),
    "fast128-nk": (700, 264, 200, 0, 0, False),
    "fast128-kn": (700, 264, 200, 1, 0, False),
    "gg8-nk": (700, 264, 200, 0, 2, False),
    "gg8-kn": (700, 264, 200, 1, 2, False),
    "gg4-nk": (700, 520, 256, 0, 4, False),
}


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_contract(name):
    M, N, Kd, layout, kernel, generic = DENSE[name]
    g = torch.Generator().manual_seed(11)
    A = G.rows_a(M, Kd, g)
    B = G.weights_b((N, Kd) if layout == 0 else (Kd, N), g)
    acc = A.double() @ (B.double().t() if layout == 0 else B.double())
    bias, bias32 = G.bias_bf16(N, g), G.bias_f32(N, g)
    aux = G.aux_grid((M, N), g)
    dA, dB, dbias, dbias32, daux = A.to(BF).to(DEV), B.to(BF).to(DEV), bias.to(DEV), bias32.to(DEV), aux.to(DEV)
    assert G.count_ties(acc) > 20
    for epi, act, opt in _cases(False):
        if epi == G.ROWSCALE:
            continue                                      # a csmoe_grouped_gemm epilogue
        what = f"dense {name} {G.EPI_NAMES[epi]} act={G.ACT_NAMES[act]} {opt}"
        b = opt.get("bias", "bf16")
        bt = None if b is None else (dbias if epi in (G.BIAS, G.BIAS_ACT) else dbias32 if epi == G.R32_ACT else None)
        want_c2 = epi in (G.BIAS_ACT, G.R32_ACT)
        res = ops.dense_gemm(dA, dB, layout, bias=bt, epilogue=epi, act=act, aux=daux if epi == G.ACTGRAD else None, want_c2=want_c2,
                             force_generic=generic, want_c=opt.get("want_c", True), kernel=kernel)
        C, C2 = res if want_c2 else (res, None)
        kw = {}
        if bt is not None:
            kw["bias"] = (bias.float() if epi != G.R32_ACT else bias32)[None, :].expand(M, N)
        if epi == G.ACTGRAD:
            kw["aux"] = aux
        ref = G.epilogue_ref(acc, epi, act, **kw)
        for out, t in (("C", C), ("C2", C2)):
            if t is not None:
                G.compare(t, ref[out], G.is_exact(epi, act, out), gelu=act in G.GELU_FAMILY, g=ref.get("g"), what=f"{what} {out}")
    # ACCUM: C = round(C + round(acc)) into a strided view, columns past N untouched
    c0 = G.aux_grid((M, N), g)
    buf = torch.full((M, N + 8), CANARY, dtype=BF, device=DEV)
    buf[:, :N] = c0.to(DEV)
    view = buf[:, :N]
    ops.dense_gemm(dA, dB, layout, epilogue=G.ACCUM, force_generic=generic, kernel=kernel, out=view)
    G.compare(view, G.epilogue_ref(acc, G.ACCUM, c_in=c0)["C"], True, what=f"dense {name} ACCUM")
    assert bool((buf[:, N:].cpu() == CANARY).all()), f"dense {name} ACCUM wrote past N"
    if kernel in (2, 4) and not generic:
        _check_softplus(name, dA, dB, layout, kernel, acc, bias, dbias, g)


def _check_softplus(name, dA, dB, layout, kernel, acc, bias, dbias, g):
    """SOFTPLUS_ROWSUM (fp32 table [M, ceil(N/256)], ldc = its row stride + 1 canary column) and SOFTPLUS_GRAD, all flag values."""
    M, N = acc.shape
    nt = (N + 255) // 256
    daff = (torch.randint(-64, 65, (M,), generator=g).float() / 16 + 2.0 ** -20).to(DEV)
    for flags in range(4):
        for bt in (None, dbias):
            what = f"dense {name} SOFTPLUS flags={flags} bias={bt is not None}"
            tab = torch.full((M, nt + 1), CANARY, dtype=F32, device=DEV)
            L.check(L.lib.csmoe_dense_gemm(dA.data_ptr(), dA.stride(0), dB.data_ptr(), layout, dB.stride(0),
                                           None if bt is None else bt.data_ptr(), M, N, dA.shape[1], tab.data_ptr(), None, None, nt + 1,
                                           G.SP_ROWSUM, flags, L.BF16, kernel, _stream()), what)
            terms = G.softplus_terms(acc, None if bt is None else bias, flags)
            t = tab.cpu()
            assert bool((t[:, nt] == CANARY).all()), f"{what}: table column past ceil(N/256) written"
            for j in range(nt):
                tt = terms[:, 256 * j: 256 * (j + 1)]
                extra = 2.0 ** -19 * tt.abs().sum(1).double()
                if flags & 2:
                    extra = extra + 2 * G.ulp_bf16(tt).max(1).values.double()
                G.check_fp32_sums(t[:, j], tt, f"{what} tile {j}", extra=extra)
            dy = torch.empty(M, N, dtype=BF, device=DEV)
            L.check(L.lib.csmoe_dense_gemm(dA.data_ptr(), dA.stride(0), dB.data_ptr(), layout, dB.stride(0),
                                           None if bt is None else bt.data_ptr(), M, N, dA.shape[1], dy.data_ptr(), None, daff.data_ptr(),
                                           N, G.SP_GRAD, flags, L.BF16, kernel, _stream()), what)
            ref, _ = G.softplus_grad_ref(acc, None if bt is None else bias, daff.cpu(), flags)
            G.compare(dy, ref, False, what=what + " GRAD")


# ------------------------------------------------------------------------------------------------ the tiled kernels agree
@pytest.mark.parametrize("layout", [0, 1])
def test_tiled_kernels_agree(layout):
    """The 128-tile, 8-wave and one-wave-per-SIMD kernels (and, KN, the fp32-master path) share the fast formulas: every epilogue and
    activation must give the same bits on the same operands."""
    o = Operands(ROWS_128 + [256 + 64], 264, 256, layout, BF, seed=21)
    kernels = [0, 2, 4] if layout == 0 else [0, 2]
    assert ops.rowdot_cols(o.M, o.N, o.Kd, o.lda, o.Kd if layout == 0 else o.N, o.ldc, BF) == o.N // 8     # kernel 0 -> 128-tile
    B32 = torch.stack(o.B).to(DEV) if layout == 1 else None
    for epi, act, opt in _cases(False):
        kw = {k: v for k, v in opt.items() if k != "dot"}
        outs = []
        for k in kernels:
            rc, C, C2 = grouped(o, epi, act, k, **kw)
            assert rc == 0, L.lib.csmoe_last_error().decode()
            outs.append((k, C, C2))
        if layout == 1 and epi != G.ROWSCALE:
            C = o.out_buf() if kw.get("want_c", True) else None
            C2 = o.out_buf() if epi in (G.BIAS_ACT, G.R32_ACT) else None
            b = kw.get("bias", "bf16")
            bias = None if b is None else (o.dbiasp if epi in (G.BIAS, G.BIAS_ACT) else o.dbias32p if epi == G.R32_ACT else None)
            L.check(L.lib.csmoe_grouped_gemm_f32w(o.dA.data_ptr(), o.lda, ops.ptr_table(B32, o.E, o.Kd * o.N * 4).data_ptr(), o.N, None,
                                                  None if bias is None else bias.data_ptr(), o.doff.data_ptr(), o.E, o.M, o.N, o.Kd,
                                                  None if C is None else C.data_ptr(), None if C2 is None else C2.data_ptr(),
                                                  o.daux.data_ptr() if epi == G.ACTGRAD else None, o.ldc, epi, act, _stream()), "f32w")
            outs.append(("f32w", C, C2))
        torch.cuda.synchronize()
        k0, C0, C20 = outs[0]
        for k, C, C2 in outs[1:]:
            for a, b_, out in ((C0, C, "C"), (C20, C2, "C2")):
                if a is not None:
                    ok = torch.equal(_bits(a[:o.used, :o.N]), _bits(b_[:o.used, :o.N]))
                    if not ok:
                        i = (_bits(a[:o.used, :o.N]) != _bits(b_[:o.used, :o.N])).nonzero()[0].tolist()
                        raise AssertionError(f"{G.EPI_NAMES[epi]} act={G.ACT_NAMES[act]} {opt} {out}: kernel {k0} and {k} differ at {i}")


# ------------------------------------------------------------------------------------------------ dot table vs kernel selector
def test_rowdot_kernel_selector():
    """rowdot_cols does not take `kernel`: below M = 2048 it reports the 128-tile layout [M][N/8].  kernel = 2 / 4 runs a 256x256 kernel
    there, which writes [M][ceil(N/128)]: such a launch is refused before anything is launched; without a table it runs."""
    o = Operands([0, 300, 400, 0], 264, 256, 0, BF, seed=5)
    cols = ops.rowdot_cols(o.M, o.N, o.Kd, o.lda, o.Kd, o.ldc, BF)
    assert cols == o.N // 8
    for kernel in (2, 4):
        dot = torch.full((o.M, cols), CANARY, dtype=F32, device=DEV)
        rc, C, _ = grouped(o, G.ROWSCALE, G.RELU, kernel, dot=dot)
        torch.cuda.synchronize()
        assert rc == 3, (kernel, rc)
        assert "rowdot_cols" in L.lib.csmoe_last_error().decode()
        assert bool((C.cpu() == CANARY).all()) and bool((dot.cpu() == CANARY).all()), "a refused launch wrote"
        rc, C, _ = grouped(o, G.ROWSCALE, G.RELU, kernel)
        torch.cuda.synchronize()
        assert rc == 0
        G.compare(C[:o.used, :o.N], _ref(o, G.ROWSCALE, G.RELU)["C"], True, what=f"kernel {kernel} without a table")
    dot = torch.full((o.M, cols), CANARY, dtype=F32, device=DEV)
    rc, _, _ = grouped(o, G.ROWSCALE, G.RELU, 0, dot=dot)
    torch.cuda.synchronize()
    assert rc == 0
    G.check_fp32_sums(dot.cpu()[:o.used].double().sum(1), _ref(o, G.ROWSCALE, G.RELU)["dot_terms"], "kernel 0 dot table")


# ------------------------------------------------------------------------------------------------ weight gradients
WGRAD = {
    # name: (counts, Na, Nb, force_generic, expected kernel family)
    "generic": ([0, 1, 65, 200, 0], 136, 72, True),
    "fast128": ([0, 1, 65, 200, 129, 0], 264, 136, False),
    "gg8w": ([0, 1, 65, 300, 700, 129, 0], 264, 520, False),
}


def _wgrad_operands(counts, Na, Nb, seed):
    g = torch.Generator().manual_seed(seed)
    off = _offsets(counts)
    M = int(off[-1])
    A = G.rows_a(M, Na, g)
    B = G.weights_b((M, Nb), g)
    return off, A, B


def _wgrad_run(name, A, B, off, Na, Nb, out_dtype, accumulate, generic, xcd, P):
    E = len(off) - 1
    offd = off.to(DEV)
    if P > 1:
        offd = ops.chunk_offsets(offd, E, P, 1)
        off = offd.cpu()
        E = E * P
    ldc = Nb + 8
    g = torch.Generator().manual_seed(3)
    old = G.aux_grid((E, Na, Nb), g)
    buf = torch.full((E, Na, ldc), CANARY, dtype=out_dtype)
    if accumulate:
        buf[:, :, :Nb] = old.to(out_dtype)
    dbuf = buf.to(DEV)
    ptrs = ops.ptr_table(dbuf, E, Na * ldc * dbuf.element_size())
    order = ops.expert_order(offd, E) if xcd else None
    dA, dB = A.to(BF).to(DEV), B.to(BF).to(DEV)
    L.check(L.lib.csmoe_grouped_wgrad(dA.data_ptr(), Na, dB.data_ptr(), Nb, offd.data_ptr(), E, A.shape[0], Na, Nb, ptrs.data_ptr(), ldc,
                                      L.BF16, L.F32 if out_dtype == F32 else L.BF16, int(accumulate), int(generic),
                                      None if order is None else order.data_ptr(), _stream()), name)
    out = dbuf.cpu()
    what = f"wgrad {name} out={out_dtype} acc={accumulate} xcd={xcd} P={P}"
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        acc = A[r0:r1].double().t() @ B[r0:r1].double()
        want = G.wgrad_ref(acc, out_dtype, old[e].to(out_dtype) if accumulate else None)
        G.compare(out[e, :, :Nb], want, True, dtype=out_dtype, what=f"{what} expert {e} rows {r1 - r0}")
        assert torch.equal(_bits(out[e, :, Nb:]), _bits(torch.full((Na, 8), CANARY, dtype=out_dtype))), f"{what}: columns past Nb written"


@pytest.mark.parametrize("name", list(WGRAD))
def test_wgrad_contract(name):
    counts, Na, Nb, generic = WGRAD[name]
    off, A, B = _wgrad_operands(counts, Na, Nb, seed=len(name))
    for out_dtype in (F32, BF):
        for accumulate in (False, True):
            _wgrad_run(name, A, B, off, Na, Nb, out_dtype, accumulate, generic, False, 1)
    if name == "gg8w":
        for xcd, P in ((True, 1), (False, 3), (True, 3)):
            _wgrad_run(name, A, B, off, Na, Nb, F32, xcd and P == 1, generic, xcd, P)
            _wgrad_run(name, A, B, off, Na, Nb, BF, False, generic, xcd, P)


@pytest.mark.parametrize("M,Na,Nb,generic", [(333, 136, 72, True), (333, 264, 136, False), (900, 264, 520, False)])
def test_dense_wgrad_contract(M, Na, Nb, generic):
    g = torch.Generator().manual_seed(M + Na)
    A, B = G.rows_a(M, Na, g), G.weights_b((M, Nb), g)
    acc = A.double().t() @ B.double()
    for od in (F32, BF):
        got = ops.dense_wgrad(A.to(BF).to(DEV), B.to(BF).to(DEV), out_dtype=od, force_generic=generic)
        G.compare(got, G.wgrad_ref(acc, od), True, dtype=od, what=f"dense_wgrad {M}x{Na}x{Nb} generic={generic} out={od}")


# ------------------------------------------------------------------------------------------------ random data, tight bound
RANDOM = {
    # name: (E, M, N, Kd, layout, kernel, generic)
    "generic16-nk": (3, 600, 136, 1032, 0, 0, True),
    "fast128-nk": (3, 1500, 264, 2048, 0, 0, False),
    "fast128-kn": (3, 1500, 264, 1032, 1, 0, False),
    "gg8-nk": (3, 2100, 264, 1544, 0, 2, False),
    "gg8-kn": (3, 2100, 264, 3000, 1, 2, False),
    "gg4-nk": (3, 2100, 520, 4096, 0, 4, False),
    "f32w-kn": (3, 2100, 264, 1024, 1, 0, False),
}


@pytest.mark.parametrize("name", list(RANDOM))
def test_random_data_bound(name):
    E, M, N, Kd, layout, kernel, generic = RANDOM[name]
    g = torch.Generator().manual_seed(len(name) + Kd)
    off = _offsets([M // 3, M - M // 3 - 7, 7])
    A = torch.randn(M, Kd, generator=g).bfloat16()
    shape = (N, Kd) if layout == 0 else (Kd, N)
    B32 = [torch.randn(*shape, generator=g) / Kd ** 0.5 for _ in range(E)]
    Bs = [b.bfloat16() for b in B32]
    dA = A.to(DEV)
    if name.startswith("f32w"):
        C = ops.grouped_gemm_f32w(dA, torch.stack(B32).to(DEV), off.to(DEV)).cpu()
    else:
        dBs = [b.to(DEV) for b in Bs]                  # kept alive: the pointer table does not hold the tensors
        C = ops.grouped_gemm(dA, ops.ptr_array(dBs, DEV), layout, Bs[0].stride(0), N, off.to(DEV), E, force_generic=generic,
                             kernel=kernel).cpu()
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        Bk = Bs[e].t() if layout == 0 else Bs[e]
        ok, worst = gemm_bound_ok(C[r0:r1], A[r0:r1], Bk)
        assert ok, f"{name} expert {e}: beyond the fp64 bound by {worst}"
    # the weight gradient of the same rows (A^T @ C-shaped operand), on the kernel the shape selects
    if name in ("generic16-nk", "fast128-nk", "gg8-nk"):
        Bw = torch.randn(M, N, generator=g).bfloat16()
        W = ops.dense_wgrad(dA, Bw.to(DEV), out_dtype=F32, force_generic=generic).cpu()
        ok, worst = gemm_bound_ok(W, A.t(), Bw)
        assert ok, f"{name} dense_wgrad: beyond the fp64 bound by {worst}"


# ------------------------------------------------------------------------------------------------ process-wide switches
@functools.lru_cache(maxsize=None)
def _menu_operands(layout):
    return Operands(ROWS_256, 264, 256, layout, BF, seed=31 + layout)


def _menu():
    """A fixed set of launches whose kernel or loop the process switches change; returns {key: CPU tensor}."""
    out = {}
    for layout in (0, 1):
        o = _menu_operands(layout)
        for kernel in (0, 2) if layout == 1 else (0, 2, 4):
            for epi, act, opt in ((G.PLAIN, 0, {}), (G.BIAS_ACT, G.GELU, {}), (G.BIAS_ACT, G.SILU, {}), (G.R32_ACT, G.RELU, {}),
                                  (G.ACTGRAD, G.GELU, {}), (G.ROWSCALE, G.QUICK_GELU, {})):
                rc, C, C2 = grouped(o, epi, act, kernel, **opt)
                assert rc == 0, L.lib.csmoe_last_error().decode()
                out[f"g{layout}.{kernel}.{epi}.{act}.C"] = C.cpu()
                if C2 is not None:
                    out[f"g{layout}.{kernel}.{epi}.{act}.C2"] = C2.cpu()
        if layout == 1:
            for copy in (False, True):
                cbuf = torch.zeros(o.E, o.Kd, o.N, dtype=BF, device=DEV) if copy else None
                res = ops.grouped_gemm_f32w(o.dA[:, :o.Kd].contiguous(), torch.stack(o.B).to(DEV), o.doff, copy=cbuf,
                                            bias_ptrs=o.dbiasp, epilogue=G.BIAS_ACT, act=G.GELU, want_c2=True)
                out[f"f32w.{copy}.C"], out[f"f32w.{copy}.C2"] = res[0][:o.used].cpu(), res[1][:o.used].cpu()
    off, A, B = _wgrad_operands([0, 1, 65, 300, 700, 129, 0], 264, 520, seed=4)
    offd = off.to(DEV)
    for xcd in (False, True):
        w = torch.zeros(7, 264, 520, device=DEV)
        ops.grouped_wgrad(A.to(BF).to(DEV), B.to(BF).to(DEV), offd, 7, w, ops.ptr_table(w, 7, 264 * 520 * 4),
                          xcd_order=ops.expert_order(offd, 7) if xcd else None)
        out[f"wgrad.{xcd}"] = w.cpu()
    torch.cuda.synchronize()
    return out


def _menu_save(path):
    torch.save(_menu(), path)


def _menu_ref(key, out):
    """Reference check of one default-run output of _menu."""
    if key.startswith("wgrad"):
        off, A, B = _wgrad_operands([0, 1, 65, 300, 700, 129, 0], 264, 520, seed=4)
        for e in range(7):
            r0, r1 = int(off[e]), int(off[e + 1])
            G.compare(out[e], G.wgrad_ref(A[r0:r1].double().t() @ B[r0:r1].double(), F32), True, dtype=F32, what=f"{key} expert {e}")
        return
    if key.startswith("f32w"):
        o = _menu_operands(1)
        ref = _ref(o, G.BIAS_ACT, G.GELU)
        part = key.rsplit(".", 1)[1]
        G.compare(out[:o.used], ref[part], part == "C", gelu=True, g=ref.get("g"), what=key)
        return
    lay, kernel, epi, act, part = key[1:].split(".")
    o = _menu_operands(int(lay))
    epi, act = int(epi), int(act)
    ref = _ref(o, epi, act)
    _check_out(o, out, ref, epi, act, part, key)


SWITCHES = {
    "sched2-thin0-split0-persist0": {"CSMOE_GEMM_SCHED": "2", "CSMOE_THIN_LOOP": "0", "CSMOE_F32W_SPLIT": "0", "CSMOE_GEMM_PERSISTENT": "0"},
    "sched3-kernel-v1": {"CSMOE_GEMM_SCHED": "3", "CSMOE_GEMM_KERNEL": "v1"},
}
_SWITCH_VARS = ("CSMOE_GEMM_SCHED", "CSMOE_THIN_LOOP", "CSMOE_F32W_SPLIT", "CSMOE_GEMM_PERSISTENT", "CSMOE_GEMM_KERNEL")


def _child(code, args, env_extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in _SWITCH_VARS}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code, *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_process_switches(tmp_path):
    """Each switch is read once per process: the switched runs go to fresh children, one at a time, and must give the default run's
    bits, which are checked against the reference here."""
    if any(os.environ.get(k) for k in _SWITCH_VARS):
        pytest.fail("run the suite without CSMOE_GEMM_* / CSMOE_THIN_LOOP / CSMOE_F32W_SPLIT set")
    default = _menu()
    for key, t in default.items():
        _menu_ref(key, t)
    code = "import sys; from tests.test_gemm_conformance_gpu import _menu_save; _menu_save(sys.argv[1])"
    for tag, env in SWITCHES.items():
        f = str(tmp_path / f"{tag}.pt")
        _child(code, [f], env)
        got = torch.load(f, weights_only=True)
        assert set(got) == set(default), tag
        for k in default:
            if not torch.equal(_bits(got[k]), _bits(default[k])):
                i = (_bits(got[k]) != _bits(default[k])).nonzero()[0].tolist()
                raise AssertionError(f"{tag}: {k} differs from the default run at {i}")


# ------------------------------------------------------------------------------------------------ LDS attribute per instantiation
_LDS_CHILD = r"""
import torch
from competesmoe_amd import ops, _lib as L
from tests import gemm_contract as G
dev = "cuda"
g = torch.Generator().manual_seed(1)
M, N, Kd = 600, 264, 256
A = G.rows_a(M, Kd, g)
Bnk = G.weights_b((N, Kd), g)
Bkn = G.weights_b((Kd, N), g)
c0 = G.aux_grid((M, N), g)
dA = A.to(torch.bfloat16).to(dev)
def check(got, acc, what, c_in=None):
    ref = G.epilogue_ref(acc, G.ACCUM if c_in is not None else G.PLAIN, c_in=c_in)["C"]
    G.compare(got, ref, True, what=what)
acc_nk = A.double() @ Bnk.double().t()
acc_kn = A.double() @ Bkn.double()
# the ACCUM instantiations first: before the fix their launch set the attribute flag every other instantiation of the kernel shares
for kernel in (2, 4):
    out = c0.to(dev)
    ops.dense_gemm(dA, Bnk.to(torch.bfloat16).to(dev), 0, epilogue=G.ACCUM, kernel=kernel, out=out)
    check(out, acc_nk, f"ACCUM kernel {kernel}", c_in=c0)
for kernel in (2, 4, 0):
    check(ops.dense_gemm(dA, Bnk.to(torch.bfloat16).to(dev), 0, kernel=kernel), acc_nk, f"NK kernel {kernel}")
for kernel in (2, 0):
    check(ops.dense_gemm(dA, Bkn.to(torch.bfloat16).to(dev), 1, kernel=kernel), acc_kn, f"KN kernel {kernel}")
out = c0.to(dev)
ops.dense_gemm(dA, Bkn.to(torch.bfloat16).to(dev), 1, epilogue=G.ACCUM, kernel=2, out=out)
check(out, acc_kn, "ACCUM KN kernel 2", c_in=c0)
B2 = G.weights_b((M, N), g)
for Na in (136, 256):
    w = ops.dense_wgrad(dA[:, :Na].contiguous(), B2.to(torch.bfloat16).to(dev), out_dtype=torch.float32)
    G.compare(w, (A[:, :Na].double().t() @ B2.double()).float(), True, dtype=torch.float32, what=f"wgrad Na={Na}")
torch.cuda.synchronize()
print("ok")
"""


def test_lds_attribute_per_instantiation():
    """hipFuncAttributeMaxDynamicSharedMemorySize is set per kernel instantiation (csrc/common.h set_dyn_lds, one flag per kernel): a fresh
    process launches EPI_ACCUM first on gg8_kernel
    and gg4_kernel, then the other instantiations (and the 128-tile / weight-gradient kernels), and checks every result exactly."""
    r = _child(_LDS_CHILD, [], {})
    assert r.stdout.strip().endswith("ok")
