"""Reference of the GEMM epilogue contract of include/csmoe.h (CSMOE_EPI_*), on exact data.

A plain helper module (no fixtures, no GPU): the data generator and one reference function per epilogue, written from the text of
csmoe.h with torch fp32 / bf16 tensor ops.  `.bfloat16()` rounds to nearest even, as the device conversion does.

Exactness argument.  A holds integers in [-4, 4] times a power-of-two scale per row (2^0 .. 2^-6), B integers in [-4, 4] times 2^-6.
Every product is a multiple of 2^-12 of magnitude <= 16 * 2^-6, so with Kd <= 2048 every partial sum is a multiple of 2^-12 below
2048 * 2^-2 = 2^9: 21 significant bits, which fp32 holds exactly.  The fp32 accumulator is then exact for ANY summation order (the
order inside an MFMA included), every kernel's accumulator equals the fp64 product, and any difference that remains is an epilogue
difference.  The same holds for the weight gradients (the reduction runs over <= 2048 binned rows of the same grid).

The data also exercises the rounding itself: an unscaled row's accumulator is a multiple of 2^-6; in [4, 8) bf16 keeps multiples of
2^-5, so every odd multiple of 2^-6 there is an exact tie of the bf16 conversion (9 significant bits, the last one set).  Unscaled
rows at Kd ~ 1k land there often; `count_ties` lets a test assert that ties occurred.  The row scales put the activation inputs across
[-8, 8]; bf16 biases have fraction bits, fp32 biases have bits below bf16 resolution, the fp32 row scales of ACTGRAD_ROWSCALE are not
bf16-representable, and `aux` is a bf16 grid over [-8, 8] that includes 0 and negative values.

Comparison classes (`compare`):
  exact           torch.equal -- every C of PLAIN / BIAS / BIAS_ACT / ROUND_BIAS32_ACT, every output with NONE or ReLU, ACCUM,
                  ACTGRAD and ROWSCALE with ReLU, all weight-gradient outputs;
  transcendental  each element within 1 bf16 ulp of the reference, plus |g| * 2^-21 for the GELU family (g = the rounded factor that
                  multiplies the activation or its derivative, 1 for C2: the fast erf's absolute error of 1.5e-7 deep in the negative
                  tail is larger than an ulp there), and at most 2 % of a case's elements may differ at all (counted where that
                  allowance is below half an ulp: in the tail a flip is the expected outcome of the documented error);
                  act and act' come from torch's formulas evaluated in fp64 and rounded once to fp32;
  fp32 sums       the ROWSCALE dot table and SOFTPLUS_ROWSUM add many fp32 terms: each row is checked against an fp64 sum of the same
                  rounded terms within n * 2^-23 * sum |term| (n = number of terms).  The softplus terms come from exp / log (the
                  hardware approximations unless flag bit 0 is set), so that check adds 2^-19 sum |term| and, with the terms rounded
                  to bf16 (flag bit 1), two bf16 ulps of the largest term: a term next to a rounding boundary may round the other way.
The fp32 generic kernel rounds nowhere; its transcendental outputs are held to 2^-14 relative (+ |g| * 2^-21).

Observed on an MI355X (test_gemm_conformance_gpu.py, all kernels, epilogues and activations; maximum over the cases):
  exact class      no difference anywhere.
  bf16, outside GELU's tail: largest difference 1 ulp; mismatch rate GELU 0.11 %, GELU_TANH 0.36 %, SiLU 0.0015 %, quick-GELU 0.026 %.
  bf16, GELU / GELU_TANH tail (|g| 2^-21 above half an ulp): up to 255 ulps of results smaller than that allowance, all within it.
  fp32 generic kernel: relative difference up to 1e-6 (SiLU) and 2.8e-5 (quick-GELU's hardware exp at 1.702 x) outside the GELU
  tails; about half of the transcendental outputs differ in their last bits.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

BF = torch.bfloat16

# epilogue / activation codes (include/csmoe.h; duplicated here so that the module imports without the HIP library)
PLAIN, BIAS, BIAS_ACT, ACTGRAD, R32_ACT, SP_ROWSUM, SP_GRAD, ROWSCALE, ACCUM = 0, 1, 2, 3, 4, 5, 6, 7, 8
NONE, RELU, GELU, GELU_TANH, SILU, QUICK_GELU = 0, 1, 2, 3, 4, 5
ACTS = (NONE, RELU, GELU, GELU_TANH, SILU, QUICK_GELU)
ACT_NAMES = {NONE: "none", RELU: "relu", GELU: "gelu", GELU_TANH: "gelu_tanh", SILU: "silu", QUICK_GELU: "quick_gelu"}
EPI_NAMES = {PLAIN: "PLAIN", BIAS: "BIAS", BIAS_ACT: "BIAS_ACT", ACTGRAD: "ACTGRAD", R32_ACT: "ROUND_BIAS32_ACT",
             SP_ROWSUM: "SOFTPLUS_ROWSUM", SP_GRAD: "SOFTPLUS_GRAD", ROWSCALE: "ACTGRAD_ROWSCALE", ACCUM: "ACCUM"}
GELU_FAMILY = (GELU, GELU_TANH)


# ------------------------------------------------------------------------------------------------ exact data
def rows_a(M: int, Kd: int, g: torch.Generator) -> torch.Tensor:
    """[M, Kd] fp32 holding bf16-exact values: integers in [-4, 4] times 2^-s per row, s in 0..6 (half the rows unscaled)."""
    a = torch.randint(-4, 5, (M, Kd), generator=g).float()
    s = torch.randint(0, 7, (M, 1), generator=g)
    s[torch.rand(M, 1, generator=g) < 0.5] = 0
    return a * torch.pow(2.0, -s.float())


def weights_b(shape, g: torch.Generator) -> torch.Tensor:
    """fp32 values on the grid integers in [-4, 4] times 2^-6 (bf16-exact)."""
    return torch.randint(-4, 5, tuple(shape), generator=g).float() * 2.0 ** -6


def bias_bf16(n: int, g: torch.Generator) -> torch.Tensor:
    """bf16 biases with fraction bits: multiples of 2^-5 in [-2, 2] (sums with the accumulator stay exact in fp32)."""
    return (torch.randint(-64, 65, (n,), generator=g).float() * 2.0 ** -5).to(BF)


def bias_f32(n: int, g: torch.Generator) -> torch.Tensor:
    """fp32 biases in [-1, 1] with bits below bf16 resolution (multiples of 2^-20)."""
    return torch.randint(-(1 << 20), (1 << 20) + 1, (n,), generator=g).float() * 2.0 ** -20


def row_scales(m: int, g: torch.Generator) -> torch.Tensor:
    """fp32 row scales in [0.5, 2) that bf16 cannot represent (random low mantissa bits)."""
    s = 1.0 + torch.randint(1, 1 << 23, (m,), generator=g).double() * 2.0 ** -23
    s = s * torch.pow(2.0, torch.randint(-1, 1, (m,), generator=g).double())
    return s.float()


def aux_grid(shape, g: torch.Generator) -> torch.Tensor:
    """bf16 pre-activations on the grid k / 8, k in [-64, 64]: includes 0 and negative values."""
    return (torch.randint(-64, 65, tuple(shape), generator=g).float() / 8).to(BF)


def count_ties(acc: torch.Tensor) -> int:
    """Accumulator values that are exact ties of the bf16 conversion (halfway between two bf16 neighbours)."""
    a = acc.float()
    lo = a.to(BF).float()
    # a tie is exactly half an ulp from the rounded value: doubling the distance gives the ulp of that binade
    d = (a - lo).abs()
    ulp = ulp_bf16(lo)
    return int(((d > 0) & (2 * d == ulp)).sum())


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """ulp of bf16 values (fp32 tensor of bf16-exact values); the smallest normal's ulp for 0 and subnormals."""
    ax = x.float().abs().clamp_min(2.0 ** -126)
    e = torch.floor(torch.log2(ax))
    return torch.pow(2.0, e - 7)


# ------------------------------------------------------------------------------------------------ activations (torch fp32)
def quick_gelu_fwd(x: torch.Tensor, dtype=BF) -> torch.Tensor:
    """x * sigmoid(1.702 x) as the reference computes it on x.dtype tensors, three ops, 1.702 x and the sigmoid rounded to `dtype`
    (common.h quick_gelu_rounded); returns the unrounded fp32 product (the caller rounds it)."""
    x = x.float()
    t = rnd(x * 1.702, dtype)
    s = rnd(torch.sigmoid(t), dtype)
    return x * s


def quick_gelu_grad(x: torch.Tensor, dtype=BF) -> torch.Tensor:
    """Derivative of quick_gelu_fwd in the rounded form of common.h quick_gelu_grad_rounded: s + 1.702 x s (1 - s)."""
    x = x.float()
    t = rnd(x * 1.702, dtype)
    s = rnd(torch.sigmoid(t), dtype)
    return s + 1.702 * x * s * (1 - s)


def _act64(x: torch.Tensor, act: int) -> torch.Tensor:
    if act == NONE:
        return x
    if act == RELU:
        return F.relu(x)
    if act == GELU:
        return F.gelu(x)
    if act == GELU_TANH:
        return F.gelu(x, approximate="tanh")
    if act == SILU:
        return F.silu(x)
    raise ValueError(act)


def act_fwd(x: torch.Tensor, act: int, dtype=BF) -> torch.Tensor:
    """act(x) of fp32 inputs: torch's formula evaluated in fp64 and rounded to fp32, i.e. the correctly rounded fp32 value (torch's
    vectorised CPU erf is an approximation with an absolute error near 1e-7 of its own, more than a bf16 ulp in GELU's negative
    tail; the reference model runs on the GPU, whose erff is accurate).  Quick-GELU: its rounded three-op form."""
    if act == QUICK_GELU:
        return quick_gelu_fwd(x, dtype)
    return _act64(x.float().double(), act).float()


def act_grad(h: torch.Tensor, act: int, dtype=BF) -> torch.Tensor:
    """act'(h) in fp32: autograd of torch's own formulas in fp64, rounded once to fp32 (see act_fwd; quick-GELU: its rounded
    closed form)."""
    h = h.float()
    if act == NONE:
        return torch.ones_like(h)
    if act == QUICK_GELU:
        return quick_gelu_grad(h, dtype)
    x = h.double().requires_grad_(True)
    with torch.enable_grad():
        y = _act64(x, act)
        (d,) = torch.autograd.grad(y.sum(), x)
    return d.detach().float()


# ------------------------------------------------------------------------------------------------ epilogues
def rnd(x: torch.Tensor, dtype) -> torch.Tensor:
    """Round to the output dtype (RNE for bf16; fp32 outputs are not rounded again), returned as fp32."""
    return x.float().to(dtype).float()


def epilogue_ref(acc: torch.Tensor, epi: int, act: int = NONE, dtype=BF, bias=None, aux=None, scale=None, c_in=None):
    """Reference of one epilogue over an exact fp32 accumulator `acc` [M, N] (fp64 or fp32 tensor of exact values).

    bias: [M, N] broadcast of each row's expert bias (bf16 values for BIAS / BIAS_ACT, fp32 for ROUND_BIAS32_ACT) or None;
    aux: [M, N] pre-activations (ACTGRAD*); scale: fp32 [M] row scales (ROWSCALE); c_in: C before an ACCUM launch.
    Returns a dict of fp32 tensors: "C" and, where the epilogue has them, "C2" (activated output), "g" (the rounded factor that
    multiplies act or act': |g| scales the GELU allowance) and "dot_terms" (ROWSCALE: round(acc) * aux, the dot table's terms)."""
    acc = acc.float()
    out = {}
    if epi == PLAIN:
        out["C"] = rnd(acc, dtype)
    elif epi in (BIAS, BIAS_ACT):
        b = bias.float() if bias is not None else torch.zeros_like(acc)
        out["C"] = rnd(acc + b, dtype)
        if epi == BIAS_ACT:
            out["C2"] = rnd(act_fwd(out["C"], act, dtype), dtype)
            out["g"] = torch.ones_like(acc)
    elif epi == R32_ACT:
        b = bias.float() if bias is not None else torch.zeros_like(acc)
        u = rnd(acc, dtype) + b                                   # fp32 add of the ROUNDED product and the fp32 bias
        out["C"] = rnd(u, dtype)
        out["C2"] = rnd(act_fwd(u, act, dtype), dtype)
        out["g"] = torch.ones_like(acc)
    elif epi == ACTGRAD:
        g = rnd(acc, dtype)
        out["C"] = rnd(g * act_grad(aux, act, dtype), dtype)
        out["g"] = g
    elif epi == ROWSCALE:
        r = rnd(acc, dtype)
        g = rnd(scale.float()[:, None] * r, dtype)
        out["C"] = rnd(g * act_grad(aux, act, dtype), dtype)
        out["g"] = g
        out["dot_terms"] = r.double() * aux.double()
    elif epi == ACCUM:
        out["C"] = rnd(c_in.float() + rnd(acc, dtype), dtype)
    else:
        raise ValueError(epi)
    return out


def softplus_terms(acc: torch.Tensor, bias, flags: int) -> torch.Tensor:
    """SOFTPLUS_ROWSUM's terms: softplus(y), y = round(acc + bias); rounded to bf16 under flag bit 1 (fp32 tensor)."""
    y = rnd(acc.float() + (bias.float()[None, :] if bias is not None else 0.0), BF)
    sp = F.softplus(y)
    return rnd(sp, BF) if flags & 2 else sp


def softplus_grad_ref(acc: torch.Tensor, bias, daff: torch.Tensor, flags: int):
    """SOFTPLUS_GRAD: C = round(g[m] * sigmoid(y)), g = daff[m] / N (rounded to bf16 under flag bit 1); returns (C, g)."""
    N = acc.shape[1]
    y = rnd(acc.float() + (bias.float()[None, :] if bias is not None else 0.0), BF)
    g = daff.float() / N
    if flags & 2:
        g = rnd(g, BF)
    g = g[:, None].expand_as(y)
    return rnd(g * torch.sigmoid(y), BF), g


def wgrad_ref(acc: torch.Tensor, out_dtype, old=None) -> torch.Tensor:
    """Weight-gradient store: round(acc) (+ the old value first when accumulating: round(old + acc))."""
    acc = acc.float()
    if old is not None:
        acc = old.float() + acc
    return rnd(acc, out_dtype)


# ------------------------------------------------------------------------------------------------ comparison
def is_exact(epi: int, act: int, out: str) -> bool:
    """Which outputs the contract fixes bit for bit (module docstring)."""
    if out == "C" and epi in (PLAIN, BIAS, BIAS_ACT, R32_ACT, ACCUM):
        return True
    return act in (NONE, RELU)


def compare(got: torch.Tensor, ref: torch.Tensor, exact: bool, gelu: bool = False, g=None, dtype=BF, what: str = ""):
    """Assert the contract's comparison class; returns (max ulp difference, mismatch fraction).  Failure messages name `what` and
    the first bad element."""
    got = got.float().cpu()
    ref = ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = (got - ref).abs()
    bad_nan = torch.isnan(got) != torch.isnan(ref)
    if exact:
        ok = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
        if not bool(ok.all()):
            i = tuple(int(v) for v in (~ok).nonzero()[0])
            raise AssertionError(f"{what}: not bit-exact at {i}: got {float(got[i])!r}, want {float(ref[i])!r} "
                                 f"({int((~ok).sum())} of {ok.numel()} differ)")
        return 0.0, 0.0
    extra = (g.float().cpu().abs() * 2.0 ** -21) if (gelu and g is not None) else (2.0 ** -21 if gelu else 0.0)
    if dtype == BF:
        ulp = ulp_bf16(ref)
        lim = ulp + extra
    else:       # nothing rounds to bf16: fp32 formulas (erff, tanhf, the hardware exp) against torch's, plus the same tail allowance
        gg = g.float().cpu().abs() if g is not None else 1.0
        lim = 2.0 ** -14 * ref.abs() + gg * 2.0 ** -21 + 1e-30
    ok = (diff <= lim) & ~bad_nan
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        raise AssertionError(f"{what}: beyond the transcendental bound at {i}: got {float(got[i])!r}, want {float(ref[i])!r}, "
                             f"bound {float(lim[i] if torch.is_tensor(lim) else lim)!r}")
    # the mismatch rate counts the elements where the tail allowance is below half an ulp; where it is larger (GELU's negative tail:
    # the fast erf's absolute error exceeds half an ulp of the tiny result) a flip is the expected outcome and the bound above governs
    counted = torch.ones_like(diff, dtype=torch.bool)
    if gelu and dtype == BF:
        counted = (extra if torch.is_tensor(extra) else torch.full_like(diff, extra)) <= ulp_bf16(ref) / 2
    frac = float(((diff != 0) & counted).sum()) / max(int(counted.sum()), 1)
    if dtype == BF:
        assert frac <= 0.02, f"{what}: {frac:.2%} of the elements differ from the reference (at most 2 % may)"
        return float((diff / ulp_bf16(ref)).max()), frac
    return float((diff / ref.abs().clamp_min(2.0 ** -126)).max()), frac


def check_fp32_sums(got: torch.Tensor, terms: torch.Tensor, what: str = "", extra=0.0):
    """Row sums of fp32 partial sums against the fp64 sum of the same terms: |got - ref| <= n 2^-23 sum |term| (n terms per row),
    + `extra` (per row) where the terms themselves come from transcendental functions."""
    got = got.double().cpu()
    terms = terms.double().cpu()
    ref = terms.sum(1)
    n = terms.shape[1]
    lim = n * 2.0 ** -23 * terms.abs().sum(1) + extra
    err = (got - ref).abs()
    if not bool((err <= lim).all()):
        i = int((err > lim).nonzero()[0])
        raise AssertionError(f"{what}: row {i}: sum {float(got[i])!r}, fp64 {float(ref[i])!r}, bound {float(lim[i])!r}")
