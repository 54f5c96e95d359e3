"""CPU checks of the GEMM contract reference (tests/gemm_contract.py): a broken reference fails here, without a GPU."""
import torch

from tests import gemm_contract as G

BF = torch.bfloat16


def test_bf16_rounding_is_nearest_even_on_ties():
    # in [4, 8) bf16 keeps multiples of 2^-5: odd multiples of 2^-6 are ties and go to the even neighbour
    x = torch.tensor([4 + 2 ** -6, 4 + 3 * 2 ** -6, -(4 + 2 ** -6), -(4 + 3 * 2 ** -6), 1 + 2 ** -8, 1 + 3 * 2 ** -8])
    want = torch.tensor([4.0, 4 + 2 ** -4, -4.0, -(4 + 2 ** -4), 1.0, 1 + 2 ** -6])
    assert torch.equal(G.rnd(x, BF), want)
    assert G.count_ties(x) == 6
    assert G.count_ties(torch.tensor([4 + 2 ** -5, 4 + 2 ** -7, 3.0])) == 0     # representable / not halfway


def test_exact_data_accumulates_exactly_and_hits_ties():
    g = torch.Generator().manual_seed(0)
    A = G.rows_a(512, 1024, g)
    B = G.weights_b((1024, 64), g)
    assert torch.equal(A.to(BF).float(), A) and torch.equal(B.to(BF).float(), B)
    acc64 = A.double() @ B.double()
    assert torch.equal((A @ B).double(), acc64)                       # fp32 accumulation is exact on this grid
    assert float(acc64.abs().max()) < 2 ** 9
    assert torch.equal(acc64 * 2 ** 12, (acc64 * 2 ** 12).round())    # multiples of 2^-12
    assert G.count_ties(acc64) > 100
    pre = acc64.abs()
    assert float(pre.max()) > 8                                       # activation inputs reach the tails


def test_round_bias32_adds_the_fp32_bias_after_rounding():
    acc = torch.tensor([[4 + 2 ** -6, 1 + 2 ** -9]], dtype=torch.float64)
    b32 = torch.tensor([[2 ** -20, 2 ** -10]])
    r = G.epilogue_ref(acc, G.R32_ACT, G.RELU, bias=b32)
    u = G.rnd(acc, BF) + b32                                          # 4 + 2^-20, 1 + 2^-10
    assert torch.equal(r["C"], G.rnd(u, BF))
    assert torch.equal(r["C2"], G.rnd(torch.relu(u), BF))
    # bias first, then rounding, gives other bits here: the order is what the reference pins
    assert not torch.equal(r["C"], G.rnd(acc.float() + b32, BF))
    # BIAS adds the bf16 bias BEFORE the rounding
    b = torch.tensor([[2 ** -6, 2 ** -9]]).to(BF)
    rb = G.epilogue_ref(acc, G.BIAS, bias=b)
    assert torch.equal(rb["C"], G.rnd(acc.float() + b.float(), BF))
    assert not torch.equal(rb["C"], G.rnd(G.rnd(acc, BF) + b.float(), BF))


def test_quick_gelu_matches_three_bf16_tensor_ops():
    x = (torch.arange(-1024, 1025, dtype=torch.float32) / 128).to(BF)
    ref = x * torch.sigmoid(1.702 * x)                                # the reference model's ops on bf16 tensors
    assert torch.equal(G.rnd(G.quick_gelu_fwd(x), BF), ref.float())
    # the derivative's closed form against autograd of the same rounded-free expression, to bf16 resolution
    xf = x.float().requires_grad_(True)
    (d,) = torch.autograd.grad((xf * torch.sigmoid(1.702 * xf)).sum(), xf)
    assert float((G.quick_gelu_grad(x) - d).abs().max()) < 2 ** -5


def test_activation_derivatives_and_rowscale_reference():
    h = torch.tensor([-2.0, -0.5, 0.0, 0.5, 3.0]).to(BF)
    assert torch.equal(G.act_grad(h, G.RELU), torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0]))
    assert torch.equal(G.act_grad(h, G.NONE), torch.ones(5))
    x = h.float()
    cdf = 0.5 * (1 + torch.erf(x / 2 ** 0.5))
    assert torch.allclose(G.act_grad(h, G.GELU), cdf + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5, atol=1e-6)
    s = torch.sigmoid(x)
    assert torch.allclose(G.act_grad(h, G.SILU), s * (1 + x * (1 - s)), atol=1e-6)
    acc = torch.tensor([[3 + 2 ** -7, -5.0]], dtype=torch.float64)
    scale = torch.tensor([1 + 2 ** -20])
    aux = torch.tensor([[1.0, 2.0]]).to(BF)
    r = G.epilogue_ref(acc, G.ROWSCALE, G.RELU, aux=aux, scale=scale)
    want = G.rnd(scale[:, None] * G.rnd(acc, BF), BF) * torch.tensor([[1.0, 1.0]])
    assert torch.equal(r["C"], want)
    assert torch.equal(r["dot_terms"], G.rnd(acc, BF).double() * aux.double())


def test_compare_classes_reject_wrong_values():
    ref = torch.tensor([1.0, 2.0, 4.0, 0.0])
    G.compare(ref.clone(), ref, exact=True)
    bumped = ref.clone()
    bumped[1] = 2 + 2 ** -6
    try:
        G.compare(bumped, ref, exact=True, what="case")
    except AssertionError as e:
        assert "case" in str(e) and "(1,)" in str(e)
    else:
        raise AssertionError("exact comparison accepted a wrong value")
    # one ulp on one element of 4 is 25 %: beyond the mismatch rate of the transcendental class
    try:
        G.compare(bumped, ref, exact=False)
    except AssertionError:
        pass
    else:
        raise AssertionError("transcendental comparison accepted a 25 % mismatch rate")
    big = torch.ones(1000)
    near = big.clone()
    near[0] = 1 + 2 ** -7
    ulps, frac = G.compare(near, big, exact=False)
    assert ulps == 1.0 and abs(frac - 0.001) < 1e-9
    G.check_fp32_sums(torch.tensor([3.0]), torch.tensor([[1.0, 2.0]]))
