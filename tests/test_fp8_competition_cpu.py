"""`args.fp8_competition` (the competition step of a pretrain `competesmoe` layer on the MXFP8 pipe) without a GPU: the constructor's
refusals, the default, and the host-side refusals of csmoe_dense_gemm_mxfp8_q / csmoe_grouped_gemm_mxfp8_q -- each returns its error
code with a message before any pointer is read and before anything is launched (the calls below pass null or made-up addresses)."""
import types

import pytest
import torch.nn.functional as F

from competesmoe_amd import _lib as L
from competesmoe_amd.pretrain import get_moe

INVALID, UNSUPPORTED = 1, 3
ARGS = dict(moe_name="competesmoe", stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
            balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False, tribrid=False,
            balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False, scale_weight=1.0, test_only=False)


def _layer(D=256, Fd=512, v_dim=None, name="competesmoe", **flags):
    args = types.SimpleNamespace(**ARGS, **flags)
    return get_moe(name)(D, 4, Fd, n_heads=2, activation=F.relu, v_dim=v_dim, log_interval=None, args=args)


def test_flag_is_off_by_default_and_a_layer_without_it_builds_as_before():
    plain = _layer()
    assert plain.fp8_competition is False and plain.fp8_experts is False
    fp8 = _layer(fp8_experts=True)
    assert fp8.fp8_competition is False and fp8.fp8_experts is True
    off = _layer(fp8_experts=True, fp8_competition=False)
    assert off.fp8_competition is False
    assert [(n, tuple(p.shape)) for n, p in off.named_parameters()] == [(n, tuple(p.shape)) for n, p in fp8.named_parameters()]
    on = _layer(fp8_experts=True, fp8_competition=True)
    assert on.fp8_competition is True
    assert [(n, tuple(p.shape)) for n, p in on.named_parameters()] == [(n, tuple(p.shape)) for n, p in fp8.named_parameters()]


def test_flag_without_fp8_experts_is_refused():
    with pytest.raises(ValueError, match="fp8_experts"):
        _layer(fp8_competition=True)


@pytest.mark.parametrize("D,Fd", [(192, 512), (256, 320), (200, 200)])
def test_reduction_dims_that_are_no_multiple_of_128_are_refused(D, Fd):
    with pytest.raises(ValueError, match="multiples of 128"):
        _layer(D=D, Fd=Fd, fp8_experts=True, fp8_competition=True)
    _layer(D=D, Fd=Fd, fp8_experts=True)                     # without the flag the layer builds as it always did


def test_output_width_that_is_no_multiple_of_8_is_refused():
    with pytest.raises(ValueError, match="multiple of 8"):
        _layer(v_dim=260, fp8_experts=True, fp8_competition=True)
    _layer(v_dim=260, fp8_experts=True)


def test_expert_parallel_layer_refuses_the_flag_after_fp8_experts():
    """competesmoe_ep refuses fp8_experts already, and that message comes first; the flag alone is refused as a single-GPU path."""
    import torch.distributed as dist
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        with pytest.raises(ValueError, match="args.fp8_experts is a single-GPU path"):
            _layer(name="competesmoe_ep", fp8_experts=True, fp8_competition=True)
        with pytest.raises(ValueError, match="fp8_competition"):
            _layer(name="competesmoe_ep", fp8_competition=True)
        with pytest.raises(ValueError, match="args.fp8_experts is a single-GPU path"):      # dims that the flag would refuse: still first
            _layer(name="competesmoe_ep", D=192, fp8_experts=True, fp8_competition=True)
    finally:
        if created:
            dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------- C ABI refusals
A, AS, B, BS, C, CQ, CS, AUX = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000     # never dereferenced


def _dense(M=64, N=64, Kd=128, C_=C, C2=None, aux=None, ldc=None, epi=L.EPI_BIAS_ACT, act=1, Cq=CQ, ldcq=None, Cs=CS, ldcs=None):
    return L.lib.csmoe_dense_gemm_mxfp8_q(A, Kd, AS, Kd // 32, B, BS, Kd, Kd // 32, None, M, N, Kd, C_, C2, aux, N if ldc is None else ldc,
                                          epi, act, Cq, N if ldcq is None else ldcq, Cs, N // 32 if ldcs is None else ldcs, None)


def _grouped(M=64, N=64, Kd=128, C_=C, C2=None, aux=None, epi=L.EPI_BIAS_ACT, act=1, Cq=CQ, ldcq=None, Cs=CS):
    return L.lib.csmoe_grouped_gemm_mxfp8_q(A, Kd, AS, Kd // 32, B, BS, Kd, Kd // 32, None, AUX, 2, M, N, Kd, C_, C2, aux, N, epi, act,
                                            Cq, N if ldcq is None else ldcq, Cs, N // 32, None)


@pytest.mark.parametrize("call", [_dense, _grouped])
def test_quantised_output_argument_rules(call):
    err = L.lib.csmoe_last_error
    assert call(Cs=None) == INVALID and b"both Cq and Cs" in err()
    assert call(Cq=None) == INVALID and b"both Cq and Cs" in err()
    for epi in (L.EPI_PLAIN, L.EPI_BIAS, L.EPI_ACTGRAD):
        assert call(epi=epi, aux=AUX) == INVALID and b"BIAS_ACT" in err()
    assert call(N=72) == UNSUPPORTED and b"N % 32" in err()
    assert call(Cq=CQ + 8) == UNSUPPORTED and b"16-byte aligned" in err()
    assert call(N=96, ldcq=104) == UNSUPPORTED and b"ldcq % 16" in err()
    assert call(Kd=192) == UNSUPPORTED and b"Kd % 128" in err()
    assert call(epi=L.EPI_ACCUM) == UNSUPPORTED and b"ACCUM" in err()
    assert call(epi=L.EPI_ACTGRAD, Cq=None, Cs=None) == INVALID and b"aux" in err()
    assert call(C_=None, Cq=None, Cs=None) == INVALID and b"null pointer" in err()         # no output at all
    assert call(M=0) == 0                                                                   # nothing to do


def test_affinity_epilogue_argument_rules():
    err = L.lib.csmoe_last_error
    assert _dense(epi=L.EPI_SOFTPLUS_GRAD, act=0, Cq=None, Cs=None) == INVALID and b"SOFTPLUS_GRAD needs aux" in err()
    assert _dense(epi=L.EPI_SOFTPLUS_ROWSUM, act=0) == INVALID and b"BIAS_ACT" in err()     # no quantised output beside them
    assert _dense(N=520, epi=L.EPI_SOFTPLUS_ROWSUM, act=0, ldc=2, Cq=None, Cs=None) == INVALID and b"ceil(N/256)" in err()
    assert _dense(epi=L.EPI_SOFTPLUS_ROWSUM, act=4, ldc=1, Cq=None, Cs=None) == INVALID and b"bad epilogue/act" in err()
    # the grouped entry has no affinity epilogues, and the entries that existed before keep refusing them
    assert _grouped(epi=L.EPI_SOFTPLUS_ROWSUM, act=0, Cq=None, Cs=None) == INVALID and b"bad epilogue/act" in err()
    assert L.lib.csmoe_dense_gemm_mxfp8(A, 128, AS, 4, B, BS, 128, 4, None, 64, 64, 128, C, None, None, 64, L.EPI_SOFTPLUS_ROWSUM, 0,
                                        None) == INVALID


def test_shape_query_states_the_rule():
    ok = lambda **k: L.lib.csmoe_gemm_mxfp8_q_ok(*[{**dict(M=64, N=64, Kd=128, lda=128, ldas=4, ldb=128, ldbs=4, ldc=64, ldcq=64, ldcs=2,
                                                         epilogue=L.EPI_BIAS_ACT, quant_out=1, dense=1), **k}[n]
                                                   for n in ("M", "N", "Kd", "lda", "ldas", "ldb", "ldbs", "ldc", "ldcq", "ldcs",
                                                             "epilogue", "quant_out", "dense")])
    assert ok() == 1
    assert ok(N=72, ldc=72, ldcq=80, ldcs=3) == 0 and ok(N=72, ldc=72, quant_out=0) == 1
    assert ok(ldcq=72) == 0 and ok(Kd=192, lda=192, ldb=192, ldas=6, ldbs=6) == 0
    assert ok(epilogue=L.EPI_PLAIN) == 0 and ok(epilogue=L.EPI_PLAIN, quant_out=0) == 1
    assert ok(N=520, ldc=3, epilogue=L.EPI_SOFTPLUS_ROWSUM, quant_out=0) == 1
    assert ok(N=520, ldc=3, epilogue=L.EPI_SOFTPLUS_ROWSUM, quant_out=0, dense=0) == 0
