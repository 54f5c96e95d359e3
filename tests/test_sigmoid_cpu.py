"""CPU checks of the sigmoid-router layers (LLaVA `smoe_sigmoidgating`, pretrain `smoe_sigmoid`): registration, constructor
signatures, state-dict names, the initial gate draw, the new rule's value, and the pin of the test-side restatement
(tests/sigmoid_ref.py) to the fixtures captured from the reference classes (tests/golden/make_golden_sigmoid.py).

bf16 sigmoid keys tie at the top-K boundary in every draw and torch.topk has no tie rule, so no row is left out and nothing depends
on which of two equal keys the reference took: on EVERY row the sorted selected keys are bitwise the reference's; on rows without a
tie among the top K + 1 keys the ids are equal in order; and with the restatement teacher-forced to the fixture's ids every later
stage is compared on all rows.  Bounds: bf16 stages bit for bit, fp32 1e-5; teacher-forced stages bf16 1e-3,
fp32 1e-5, weights bit for bit in bf16.

The backward sequence of router_select_bwd_kernel's SEL_SIGMOID_NORM branch, restated with torch ops (sigmoid_ref.
select_bwd_emulation), reproduces the restatement's autograd d gate_logits bit for bit in the bf16-quotient cases (LLaVA bf16 module,
bf16 stream) and the autocast case, and to rtol 1e-5 in fp32.  Observed on the five fixtures: 0 differing elements in every case."""
import inspect
import os
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import moe_oracle as O
from tests import sigmoid_ref as S
from tests.golden_util import load, rel_l2, max_rel

LLAVA = ["llava_smoe_sigmoidgating_fp32", "llava_smoe_sigmoidgating_bf16", "llava_smoe_sigmoidgating_e16_bf16"]
PRETRAIN = ["pretrain_smoe_sigmoid_fp32", "pretrain_smoe_sigmoid_bf16"]
E8_BF16 = ["llava_smoe_sigmoidgating_bf16", "pretrain_smoe_sigmoid_bf16"]

# parameter names of the reference constructors, in order (smoe_sigmoidgating.py:10, smoeut_norm.py:38-64)
LLAVA_SIG = ["self", "in_embed_dim", "out_embed_dim", "num_of_experts", "num_selected", "expert", "args"]
PRETRAIN_SIG = ["self", "dmodel", "n_experts", "expert_size", "n_heads", "std_gate", "std_expert", "topk", "dropout", "weight_scale",
                "selection_mode", "perplexity_reg", "perplexity_reg_mode", "activation_after_topk", "activation", "sel_bias", "bias",
                "v_dim", "expert_dropout", "sync_distributed", "selection_dropout", "log_interval", "args", "std", "out_dmodel", "is_att",
                "inp_expert", "out_expert"]


def is_bf16(fx):
    return fx["gate_logits"].dtype == torch.bfloat16


def llava_layer(fx):
    from competesmoe_amd.moe import get_moe
    m = fx["meta"]
    ex = nn.ModuleList([nn.Sequential(nn.Linear(m["D"], m["F"]), nn.GELU(), nn.Linear(m["F"], m["Dout"])) for _ in range(m["E"])])
    return get_moe("smoe_sigmoidgating")(m["D"], m["Dout"], m["E"], m["K"], ex, types.SimpleNamespace(**m["args"]))


def pretrain_layer(fx):
    from competesmoe_amd.pretrain import get_moe
    m = fx["meta"]
    return get_moe("smoe_sigmoid")(m["D"], m["E"], m["F"], n_heads=m["K"], activation=F.relu, bias=m["bias"], sel_bias=m["sel_bias"],
                                   log_interval=None, args=types.SimpleNamespace(**m["args"]))


# ------------------------------------------------------------------------------------------------ registry, signatures, state
def test_both_registries_know_the_sigmoid_router():
    from competesmoe_amd.moe import get_moe as llava_get, SMoESigmoidGating
    from competesmoe_amd.pretrain import get_moe as pre_get, SMoEUTNorm
    assert llava_get("smoe_sigmoidgating") is SMoESigmoidGating and pre_get("smoe_sigmoid") is SMoEUTNorm


def test_constructor_signatures_are_the_references():
    from competesmoe_amd.moe import SMoESigmoidGating
    from competesmoe_amd.pretrain import SMoEUTNorm
    assert list(inspect.signature(SMoESigmoidGating.__init__).parameters) == LLAVA_SIG
    sig = inspect.signature(SMoEUTNorm.__init__)
    assert list(sig.parameters) == PRETRAIN_SIG
    assert sig.parameters["selection_mode"].default == "sigmoid" and sig.parameters["std"].default == 1
    assert sig.parameters["topk"].default == 2 and sig.parameters["log_interval"].default == 100


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_state_dict_names_and_shapes_are_the_fixtures(name):
    fx = load(name)
    llava = name.startswith("llava")
    layer = llava_layer(fx) if llava else pretrain_layer(fx)
    if llava:
        layer = layer.to(fx["x"].dtype)
        assert isinstance(layer.sigmoid, nn.Sigmoid)
    assert set(layer.state_dict()) == set(fx["state"])
    layer.load_state_dict(fx["state"], strict=True)
    for k, v in layer.state_dict().items():
        assert v.shape == fx["state"][k].shape and v.dtype == fx["state"][k].dtype, k


def test_llava_gate_draw_is_the_references():
    fx = load("llava_smoe_sigmoidgating_fp32")
    layer = llava_layer(fx)
    assert layer.gate.bias is None and torch.equal(layer.gate.weight.detach(), fx["state"]["gate.weight"])


def test_header_and_lib_agree_on_the_new_rule():
    from competesmoe_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "csmoe.h")).read()
    assert "CSMOE_SEL_SIGMOID_NORM = 6" in header and _lib.SEL_SIGMOID_NORM == 6 == S.SEL_SIGMOID_NORM


# ------------------------------------------------------------------------------------------------ the restatement against the fixtures
def _forward(fx, llava, idx=None, grad=False):
    ps = {k: v.clone().requires_grad_(grad) for k, v in fx["state"].items()}
    x = fx["x"].clone().requires_grad_(grad)
    out, loss, st = (S.llava_forward if llava else S.pretrain_forward)(x, ps, fx["meta"], idx=idx)
    return x, ps, out, loss, st


def no_tie_rows(fx):
    """Rows of the fixture without an equal pair among the reference's top K + 1 keys."""
    K = fx["meta"]["K"]
    top = fx["gate_sigmoid"].float().topk(K + 1, dim=-1).values
    return ~(top[..., :-1] == top[..., 1:]).any(-1)


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_restatement_reproduces_the_router_stages_on_every_row(name):
    fx = load(name)
    llava, bf16 = name.startswith("llava"), is_bf16(fx)
    _, _, _, _, st = _forward(fx, llava)
    for k in ("gate_logits", "gate_sigmoid") + (("gate_softmax",) if llava else ()):
        a, b = st[k].detach(), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype)
        if bf16 and b.dtype == torch.bfloat16:
            assert torch.equal(a, b), (k, float((a.float() - b.float()).abs().max()))
        else:       # fp32 stages; the fp32 softmax of bf16 logits is held to the fp32 bound too
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), (k, float((a - b).abs().max()))
    ref_idx = fx["selected_experts"].long()
    mine = torch.gather(st["gate_sigmoid"].detach(), -1, st["selected_experts"]).sort(-1).values
    theirs = torch.gather(fx["gate_sigmoid"], -1, ref_idx).sort(-1).values
    assert torch.equal(mine, theirs)                                            # every row, bitwise
    clean = no_tie_rows(fx)
    assert torch.equal(st["selected_experts"][clean], ref_idx[clean])           # in order where no key ties
    share = float(clean.float().mean())
    assert abs((1.0 - share) - fx["meta"]["tie_rows"]) < 1e-9
    if not bf16:
        assert share == 1.0
    elif name in E8_BF16:
        assert share >= 0.75, share          # a condition on the fixture (the generator's seed policy), not a tolerance


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_teacher_forced_restatement_reproduces_every_later_stage(name):
    fx = load(name)
    llava, bf16 = name.startswith("llava"), is_bf16(fx)
    tol = 1e-3 if bf16 else 1e-5
    x, ps, out, loss, st = _forward(fx, llava, idx=fx["selected_experts"], grad=True)
    w, wr = st["weights"].detach(), fx["weights"]
    assert w.dtype == wr.dtype and w.shape == wr.shape
    if bf16:
        assert torch.equal(w, wr), float((w.float() - wr.float()).abs().max())
    else:
        assert float((w - wr).abs().max()) <= tol
    assert out.dtype == fx["output"].dtype

    def close(a, b, what):
        print(f"{name}: {what} rel-L2 {rel_l2(a, b):.2e} max-rel {max_rel(a, b):.2e}")
        assert rel_l2(a, b) <= tol and max_rel(a, b) <= tol, (what, rel_l2(a, b), max_rel(a, b))
    close(out.detach(), fx["output"], "output")
    if llava:
        assert abs(float(loss.detach()) - float(fx["aux_loss"])) <= tol * max(1.0, abs(float(fx["aux_loss"])))
        for k, v in fx["infor_aux"].items():
            assert abs(float(st[k]) - float(v)) <= tol * max(1.0, abs(float(v))), k
        ((out.float() * fx["dy"].float()).sum() + loss.float()).backward()
    else:
        (k, v), = fx["reg_loss"].items()
        assert k == "mlp_balance" and abs(float(loss.detach()) - float(v)) <= tol * max(1.0, abs(float(v)))
        ((out.float() * fx["dy"]).sum() + loss.float()).backward()
    close(x.grad, fx["x_grad"], "d x")
    for k, g in fx["grads"].items():
        assert g is not None and ps[k].grad is not None and ps[k].grad.dtype == g.dtype, k
        close(ps[k].grad, g, "d " + k)


# ------------------------------------------------------------------------------------------------ the kernel's backward sequence
def _loss_on_logits(fx, llava, logits, idx):
    """The losses that read the logits directly (z-loss / entropy balance), as a function of the logits alone."""
    a = fx["meta"]["args"]
    if llava:
        return O.zloss(logits) * a["router_z_loss_coef"]
    return O.entropy_balance(logits) * a["balance_loss_coef"]


@pytest.mark.parametrize("name", LLAVA + PRETRAIN)
def test_backward_emulation_gives_the_restatements_d_gate_logits(name):
    """The kernel's lines, fed the fixture's stages and the gradients the restatement's autograd puts on the weights (and on the
    softmax), plus the losses' own gradient on the logits added as GateSelect.backward adds it, against autograd's d gate_logits:
    LLaVA bf16 (bf16 quotient) and pretrain bf16 (autocast, fp32 quotient) bit for bit, fp32 rtol 1e-5."""
    fx = load(name)
    llava, bf16 = name.startswith("llava"), is_bf16(fx)
    E, K = fx["meta"]["E"], fx["meta"]["K"]
    x, ps, out, loss, st = _forward(fx, llava, idx=fx["selected_experts"], grad=True)
    for k in ("gate_logits", "weights") + (("gate_softmax",) if llava else ()):
        assert torch.equal(st[k].detach(), fx[k]) if bf16 else True
        st[k].retain_grad()
    ((out.float() * fx["dy"].float()).sum() + loss.float()).backward()
    want = st["gate_logits"].grad.reshape(-1, E)
    lg = st["gate_logits"].detach().clone().requires_grad_(True)
    _loss_on_logits(fx, llava, lg, fx["selected_experts"]).float().backward()
    logits = fx["gate_logits"].reshape(-1, E)
    sm = F.softmax(logits, dim=-1, dtype=torch.float32)
    dsm = st["gate_softmax"].grad.reshape(-1, E) if llava else None
    got = S.select_bwd_emulation(logits, sm, fx["selected_experts"].reshape(-1, K), st["weights"].grad.float().reshape(-1, K), dsm,
                                 round_sum_bf16=llava and bf16)
    got = got + lg.grad.reshape(-1, E)
    assert got.dtype == want.dtype
    print(f"{name}: d gate_logits differing elements {int((got != want).sum())} of {got.numel()}, "
          f"max |diff| {float((got.float() - want.float()).abs().max()):.2e}")
    if bf16:
        assert torch.equal(got, want)
    else:
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


@pytest.mark.parametrize("K,with_softmax", [(2, False), (2, True), (3, True)])
def test_backward_emulation_bf16_stream_and_the_two_sum_graphs(K, with_softmax):
    """The fourth way in: a bf16 stream under bf16 autocast (`sum` fp32-policy, then `.to(bf16)`), for which no layer fixture exists:
    the selection alone on the pretrain bf16 fixture's logits.  Its graph and the LLaVA bf16 module's (`sum` a bf16 tensor op) give
    the same bits, and the emulation with `round_sum_bf16` gives them too."""
    fx = load("pretrain_smoe_sigmoid_bf16")
    E = fx["meta"]["E"]
    g = torch.Generator().manual_seed(K)
    grads = []
    for sum_fp32 in (True, False):
        lg = fx["gate_logits"].reshape(-1, E).clone().requires_grad_(True)
        keys, sm, idx, w = S.select(lg, K, torch.bfloat16, sum_fp32=sum_fp32)
        assert w.dtype == torch.bfloat16
        if not grads:
            dw = torch.randn(w.shape, generator=g).bfloat16()
            dsm = torch.randn(sm.shape, generator=g) if with_softmax else None
        loss = (w * dw).sum().float()
        if with_softmax:
            loss = loss + (sm * dsm).sum()
        loss.backward()
        grads.append(lg.grad)
    assert torch.equal(grads[0], grads[1])
    got = S.select_bwd_emulation(lg.detach(), sm.detach(), idx, dw.float(), dsm, round_sum_bf16=True)
    assert torch.equal(got, grads[0]), float((got.float() - grads[0].float()).abs().max())
