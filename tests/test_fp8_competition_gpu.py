"""`args.fp8_competition`: the competition step of a pretrain `competesmoe` layer in the lean form on the MXFP8 pipe.

* functional.CompetitionAffinityPackedFP8 against the STORED fp8 form composed from functions that are checked against the MX oracle
  elsewhere (tests/test_fp8_gpu.py): DenseFFNFP8 per expert, then SoftplusMean -- the same kernels on the same quantised bytes, so
  a ReLU mask can not differ between the two.  Bounds: the affinities differ by the order of an fp32 row sum (2^-7 relative on bf16
  affinities, 2e-6 on fp32 ones: tests/test_ops_gpu.py::test_affinity_epilogues_match_gemm_then_softplus_mean); d keys / d values are
  expected bit-equal (asserted <= 5e-3 relative L2, printed); dx differs by the order of E bf16 additions (5e-3, the bound of
  tests/test_pretrain_modules_gpu.py::test_pretrain_lean_competition_backpropagates_...).
* functional.MoEFFNPackedFP8Slots against MoEFFNPackedFP8 (a row's product does not depend on its neighbours and a unit weight is
  exact, so the slot rows are the output of a K = 1 run on the repeated rows, bit for bit).
* The layer: which functions a competition step runs, that it routes by the stored-form fp8 affinities wherever their K-th and
  (K+1)-th value are 1e-5 apart (5x the re-ordering bound at affinities near 0.75; at most 2 % of rows may be closer), that its
  output is the fp8 sparse step's for that selection, and that a layer with the flag off launches what it launched before."""
import types

import pytest
import torch
import torch.nn.functional as F

from competesmoe_amd import _lib as L
from tests.golden_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

if torch.cuda.is_available():
    from competesmoe_amd import functional as Fn, ops
    from competesmoe_amd.pretrain import get_moe

T, D, FF, E, K = 320, 256, 512, 4, 2


def _masters(seed=0, n_tokens=T):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n_tokens, D, device=DEV, generator=g).to(torch.bfloat16)
    keys = torch.randn(E, D, FF, device=DEV, generator=g) * D ** -0.5
    values = torch.randn(E, FF, D, device=DEV, generator=g) * FF ** -0.5
    return x, keys, values, g


def _stored(x, keys, values, act, fp32_aff, daff=None):
    """The stored fp8 form: E dense fp8 FFNs, then the softplus-mean kernels.  (aff, dx, d keys, d values)."""
    x = x.detach().clone().requires_grad_(daff is not None)
    keys = keys.detach().clone().requires_grad_(daff is not None)
    values = values.detach().clone().requires_grad_(daff is not None)
    outs = [Fn.DenseFFNFP8.apply(x, keys[e], None, values[e], act) for e in range(E)]
    aff = torch.stack([Fn.SoftplusMean.apply(o, fp32_aff) for o in outs], dim=-1)
    if daff is None:
        return aff.detach(), None, None, None
    aff.backward(daff)
    return aff.detach(), x.grad, keys.grad, values.grad


def _lean(x, keys, values, act, fp32_aff, daff, cache=False):
    x = x.detach().clone().requires_grad_(True)
    keys = keys.detach().clone().requires_grad_(True)
    values = values.detach().clone().requires_grad_(True)
    aff = Fn.CompetitionAffinityPackedFP8.apply(x, keys, values, act, fp32_aff, cache)
    aff.backward(daff)
    return aff.detach(), x.grad, keys.grad, values.grad


def _aff_close(got, ref, fp32_aff):
    tol = 2e-6 if fp32_aff else 2.0 ** -7
    err = ((got.float() - ref.float()).abs() / ref.float().abs()).max().item()
    return err, tol


@pytest.mark.parametrize("fp32_aff", [True, False])
@pytest.mark.parametrize("act", [L.ACT_RELU, L.ACT_GELU])
def test_lean_fp8_competition_matches_the_stored_fp8_form(act, fp32_aff):
    x, keys, values, g = _masters()
    daff = torch.randn(T, E, device=DEV, generator=g).to(torch.float32 if fp32_aff else torch.bfloat16)
    ref = _stored(x, keys, values, act, fp32_aff, daff)
    got = _lean(x, keys, values, act, fp32_aff, daff)
    assert got[0].dtype == ref[0].dtype and got[0].shape == (T, E)
    err, tol = _aff_close(got[0], ref[0], fp32_aff)
    ex, ek, ev = rel_l2(got[1], ref[1]), rel_l2(got[2], ref[2]), rel_l2(got[3], ref[3])
    print(f"act={act} fp32_aff={fp32_aff}: affinity max rel err {err:.3e} (bound {tol:.3e}); dx {ex:.3e}, d keys {ek:.3e}, "
          f"d values {ev:.3e} (bound 5e-3); d keys bit-equal {torch.equal(got[2], ref[2])}, d values bit-equal "
          f"{torch.equal(got[3], ref[3])}")
    assert err <= tol
    assert float(ref[2].abs().max()) > 0 and float(ref[3].abs().max()) > 0 and float(ref[1].abs().max()) > 0
    assert ek <= 5e-3 and ev <= 5e-3
    assert ex <= 5e-3


def test_lean_fp8_competition_saves_nothing_of_the_stored_form():
    """Saved for the backward: x and the parameters -- nothing that starts [T, E] / [E, T] and no [T, F] activation."""
    x, keys, values, _ = _masters()
    x = x.requires_grad_(True)
    keys, values = keys.requires_grad_(True), values.requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        aff = Fn.CompetitionAffinityPackedFP8.apply(x, keys, values, L.ACT_RELU, True, False)
    assert aff.shape == (T, E)
    assert sorted(saved) == sorted([(T, D), (E, D, FF), (E, FF, D)]), saved
    for shp in saved:
        assert shp[:2] not in ((T, E), (E, T)) and shp != (T, FF)


def test_weight_cache_changes_no_bit_and_follows_the_version_counter():
    x, keys, values, g = _masters()
    daff = torch.randn(T, E, device=DEV, generator=g)
    Fn.fp8_weight_cache_clear()
    try:
        plain = _lean(x, keys, values, L.ACT_RELU, True, daff, cache=False)
        assert not Fn._FP8_WCACHE
        # the cache is keyed by the parameter's storage: the same tensors through both cached calls
        xk = x.detach().clone().requires_grad_(True)
        kk, vv = keys.detach().clone().requires_grad_(True), values.detach().clone().requires_grad_(True)

        def cached():
            xk.grad = kk.grad = vv.grad = None
            aff = Fn.CompetitionAffinityPackedFP8.apply(xk, kk, vv, L.ACT_RELU, True, True)
            aff.backward(daff)
            return aff.detach().clone(), xk.grad.clone(), kk.grad.clone(), vv.grad.clone()
        a = cached()
        assert len(Fn._FP8_WCACHE) == 2
        ents = {k: v[1][0][0].data_ptr() for k, v in Fn._FP8_WCACHE.items()}
        b = cached()
        assert {k: v[1][0][0].data_ptr() for k, v in Fn._FP8_WCACHE.items()} == ents          # reused, not quantised again
        for p, q, r in zip(plain, a, b):
            assert torch.equal(p, q) and torch.equal(p, r)
        with torch.no_grad():
            kk.mul_(0.5)                                      # an optimizer step: in place, bumps the version counter
        c = cached()
        assert not torch.equal(c[0], a[0])
        fresh = _lean(x, kk, vv, L.ACT_RELU, True, daff, cache=False)
        for p, q in zip(fresh, c):
            assert torch.equal(p, q)
    finally:
        Fn.fp8_weight_cache_clear()


# ------------------------------------------------------------------------------------------------ MoEFFNPackedFP8Slots
def _slot_inputs():
    Ts = 192
    x, keys, values, g = _masters(seed=1, n_tokens=Ts)
    live = torch.tensor([0, 1, 3], device=DEV)                                   # expert 2 receives no rows
    pick = torch.stack([torch.randperm(3, device=DEV, generator=g)[:K] for _ in range(Ts)])
    idx = live[pick].int().contiguous()
    w = torch.rand(Ts, K, device=DEV, generator=g) + 0.25
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    dout = torch.randn(Ts, D, device=DEV, generator=g).to(torch.bfloat16)
    dslots = torch.randn(Ts, K, D, device=DEV, generator=g).to(torch.bfloat16)
    return Ts, x, keys, values, idx, w, dout, dslots


def _run_ffn(fn, x, w, idx, keys, values, grads, act=L.ACT_RELU):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    keys, values = keys.detach().clone().requires_grad_(True), values.detach().clone().requires_grad_(True)
    res = fn.apply(x, w, idx, keys, values, None, act, L.COMBINE_DOT)
    outs = res if isinstance(res, tuple) else (res,)
    if grads is not None:
        torch.autograd.backward(list(outs), list(grads))
    return [o.detach() for o in outs], (x.grad, w.grad, keys.grad, values.grad)


def test_fp8_slots_are_the_sparse_step_plus_its_rows():
    Ts, x, keys, values, idx, w, dout, dslots = _slot_inputs()
    assert not bool((idx == 2).any())
    (ref_out,), ref_g = _run_ffn(Fn.MoEFFNPackedFP8, x, w, idx, keys, values, (dout,))
    # the slot rows: a K = 1 run on the repeated rows with unit weights
    xr, ir = x.repeat_interleave(K, 0), idx.view(-1, 1).contiguous()
    ones = torch.ones(Ts * K, 1, device=DEV)
    (rep_out,), rep_g = _run_ffn(Fn.MoEFFNPackedFP8, xr, ones, ir, keys, values, (dslots.view(Ts * K, D),))

    (out, slots), g0 = _run_ffn(Fn.MoEFFNPackedFP8Slots, x, w, idx, keys, values, (dout, torch.zeros_like(dslots)))
    assert slots.shape == (Ts, K, D)
    assert torch.equal(out, ref_out)
    assert torch.equal(slots.reshape(Ts * K, D), rep_out)
    for name, a, b in zip(("dx", "dw", "d keys", "d values"), g0, ref_g):          # a zero slot gradient adds nothing
        assert torch.equal(a, b), name

    _, g1 = _run_ffn(Fn.MoEFFNPackedFP8Slots, x, w, idx, keys, values, (torch.zeros_like(dout), dslots))
    want_dx = rep_g[0].view(Ts, K, D).float().sum(1)
    errs = (rel_l2(g1[0].float(), want_dx), rel_l2(g1[2], rep_g[2]), rel_l2(g1[3], rep_g[3]))
    print(f"slot gradient alone: dx {errs[0]:.3e}, d keys {errs[1]:.3e}, d values {errs[2]:.3e} (bound 5e-3)")
    assert float(want_dx.abs().max()) > 0
    assert max(errs) <= 5e-3, errs
    assert bool((g1[2][2] == 0).all()) and bool((g1[3][2] == 0).all())               # the expert without rows


# ------------------------------------------------------------------------------------------------ the layer
ARGS = dict(moe_name="competesmoe", stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
            balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False, tribrid=False,
            balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False, scale_weight=1.0, test_only=False)


def _layer(**flags):
    torch.manual_seed(0)
    layer = get_moe("competesmoe")(D, E, FF, n_heads=K, activation=F.relu, log_interval=None, args=types.SimpleNamespace(**ARGS, **flags))
    _, keys, values, g = _masters()
    with torch.no_grad():                     # with the layer's own init the affinities sit too close to ln 2 for a routing check
        layer.keys.copy_(keys)
        layer.values.copy_(values)
    layer = layer.to(DEV).train()
    layer.regularization_present = True
    layer.step_warm, layer.flip_steps = 0, 10
    layer.prob_flips_final = {0: torch.ones(10, dtype=torch.bool, device=DEV)}        # every step competes
    layer.set_current_steps(3)
    return layer


def _layer_x():
    g = torch.Generator(device=DEV).manual_seed(0)
    return torch.randn(2, 160, D, device=DEV, generator=g)


def _step(layer, x=None, backward=True):
    x = (_layer_x() if x is None else x).detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, id_layer=0)
        reg = layer.get_reg_loss()
    if backward:
        (out.float().pow(2).mean() + sum(v.float() for v in reg.values())).backward()
    grads = {"x": x.grad, "w_gate": layer.w_gate.grad, "keys": layer.keys.grad, "values": layer.values.grad}
    return out.detach(), reg, grads


def test_layer_competition_step_runs_lean_on_the_fp8_pipe_and_routes_by_the_fp8_affinities(monkeypatch):
    calls = {"aff8": 0, "slots8": 0, "dense": 0, "aff16": 0}

    def spy(cls, key):
        orig = cls.forward

        def f(ctx, *a):
            calls[key] += 1
            return orig(ctx, *a)
        monkeypatch.setattr(cls, "forward", staticmethod(f))
    spy(Fn.CompetitionAffinityPackedFP8, "aff8")
    spy(Fn.MoEFFNPackedFP8Slots, "slots8")
    spy(Fn.DenseFFN, "dense")
    spy(Fn.CompetitionAffinityPacked, "aff16")

    layer = _layer(fp8_experts=True, fp8_competition=True)
    picked = []
    slots0 = layer.ffn_slots

    def slots_spy(x_, sel_, w_):
        picked.append((sel_.detach().clone(), w_.detach().clone()))
        return slots0(x_, sel_, w_)
    layer.ffn_slots = slots_spy
    x = _layer_x()
    out, reg, grads = _step(layer, x)
    assert calls == {"aff8": 1, "slots8": 1, "dense": 0, "aff16": 0}, calls
    assert len(picked) == 1
    aidx, aw = picked[0]

    # the stored-form fp8 affinities of the same tokens (fp32 under autocast), and their top-K
    x2 = x.reshape(-1, D).to(torch.bfloat16)
    ref_aff, _, _, _ = _stored(x2, layer.keys.detach(), layer.values.detach(), L.ACT_RELU, True)
    top = torch.topk(ref_aff, K + 1, dim=-1)
    clear = (top.values[:, K - 1] - top.values[:, K]) >= 1e-5
    excluded = 1.0 - clear.float().mean().item()
    got = aidx.reshape(-1, K).long().sort(-1).values
    want = top.indices[:, :K].sort(-1).values
    same = (got == want).all(-1)
    print(f"routing: {excluded:.4%} of rows excluded (K-th and (K+1)-th stored-form affinity closer than 1e-5), "
          f"{(~same).float().mean().item():.4%} of all rows differ, mean affinity {ref_aff.mean().item():.4f}")
    assert excluded <= 0.02
    assert bool(same[clear].all())

    # the output is the fp8 sparse step's for the selection the layer made
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        want_out = layer.ffn(x, aidx, aw)
    assert torch.equal(out, want_out.view(out.shape))

    # same registered losses as with the flag off; finite gradients everywhere
    off = _layer(fp8_experts=True)
    _, reg_off, _ = _step(off, x)
    assert set(reg) == set(reg_off) and len(reg) >= 2
    for n, gten in grads.items():
        assert gten is not None and bool(torch.isfinite(gten.float()).all()) and float(gten.float().abs().max()) > 0, n


def test_layer_residual_from_the_block_is_added_to_the_fp8_slots_output():
    """A residual handed in by the block does not force the stored form: it is added as MoE.ffn adds it for fp8 experts, res + out."""
    layer = _layer(fp8_experts=True, fp8_competition=True)
    x = _layer_x()
    out, _, _ = _step(layer, x, backward=False)
    res = torch.randn(2, 160, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    layer._residual = res
    out_res, _, _ = _step(layer, x, backward=False)
    assert layer._residual is None
    assert torch.equal(out_res, res + out.view(res.shape))


def test_layer_weight_cache_changes_no_bit():
    res = []
    try:
        for cache in (False, True):
            Fn.fp8_weight_cache_clear()
            layer = _layer(fp8_experts=True, fp8_competition=True, fp8_weight_cache=cache)
            out, reg, grads = _step(layer)
            res.append((out, {k: v.detach().clone() for k, v in reg.items()}, grads))
            assert bool(Fn._FP8_WCACHE) == cache
    finally:
        Fn.fp8_weight_cache_clear()
    a, b = res
    assert torch.equal(a[0], b[0])
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_layer_with_the_flag_off_launches_what_it_launched_before():
    """The profile tags of one competition step (fwd + bwd) of an fp8 layer with fp8_competition = False equal those of the same
    layer built without the attribute at all -- and contain none of the new launches."""
    tags = []
    outs = []
    for flags in (dict(fp8_experts=True), dict(fp8_experts=True, fp8_competition=False)):
        layer = _layer(**flags)
        ops.profile_start()
        try:
            out, _, _ = _step(layer)
        finally:
            prof = ops.profile_stop()
        tags.append({k: v["calls"] for k, v in prof.items()})
        outs.append(out)
    assert tags[0] == tags[1], tags
    assert not [k for k in tags[0] if k.endswith("_q") or "affinity" in k], tags[0]
    assert tags[0].get("grouped_gemm_mxfp8", 0) == 4 and "dense_gemm_mxfp8" not in tags[0]      # the stored form's dense pass is bf16
    assert torch.equal(outs[0], outs[1])
    # and the flag turns them on
    layer = _layer(fp8_experts=True, fp8_competition=True)
    ops.profile_start()
    try:
        _step(layer)
    finally:
        prof = ops.profile_stop()
    assert prof["dense_gemm_mxfp8_q"]["calls"] == 2 * E                    # GEMM 1 of every expert, forward and recomputation
    assert prof["dense_gemm_affinity_mxfp8"]["calls"] == E and prof["dense_gemm_affinity_grad_mxfp8"]["calls"] == E
    assert prof["grouped_gemm_mxfp8"]["calls"] == 4                        # the sparse step's GEMM 1, GEMM 2, dH, dXs
