"""CPU (gloo): the constructor, init, schedule and rank-agreement contract of the pretrain `competesmoe_ep` layer
(competesmoe_amd/pretrain/competesmoe_ep.py).  Its forward / backward against the single-GPU layer: tests/test_pretrain_competesmoe_ep_gpu.py."""
import os
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _args(**kw):
    a = dict(stop_after=10, warm_up=0.0, rate_flip=0.5, max_compete_in_iter=8, balance_loss_coef=0.01, balance_loss_coef_comp=0.02,
             router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False, tribrid=False, balance_affinity=False,
             is_cosine=False, is_norm_weight=False, norm_sigmoid=False, scale_weight=1.0, test_only=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _launch(target, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(120)
            assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return dict(q.get(timeout=5) for _ in range(world))


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _make(D=32, E=8, F=16, bias=True, **kw):
    import torch.nn.functional as Fn
    from competesmoe_amd.pretrain import get_moe
    return get_moe("competesmoe_ep")(D, E, F, n_heads=2, activation=Fn.relu, bias=bias, log_interval=None, args=_args(), **kw)


def test_competesmoe_ep_is_registered():
    from competesmoe_amd.pretrain import EPCompeteSMoE, get_moe
    assert get_moe("competesmoe_ep") is EPCompeteSMoE


def test_competesmoe_ep_needs_a_process_group():
    with pytest.raises(RuntimeError, match="process group"):
        _make()


def _ctor_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        import torch.nn.functional as Fn
        from competesmoe_amd.pretrain import get_moe
        res = {}
        for what, kw in (("is_att", dict(is_att=True, inp_expert=32, out_expert=32)), ("fp8", dict(args=_args(fp8_experts=True))),
                         ("divide", dict(n_experts=9))):
            a = dict(dmodel=32, n_experts=8, expert_size=16, n_heads=2, activation=Fn.relu, args=_args())
            a.update(kw)
            try:
                get_moe("competesmoe_ep")(**a)
                res[what] = False
            except ValueError:
                res[what] = True
        # ranks seeded DIFFERENTLY: the replicated gate (and o_bias) still agree -- broadcast from the group's first rank
        torch.manual_seed(100 + rank)
        lay = _make()
        with torch.no_grad():
            lay.o_bias.normal_()
        lay2 = _make()
        g = [torch.empty_like(lay.w_gate) for _ in range(world)]
        dist.all_gather(g, lay.w_gate.detach())
        res["w_gate_equal"] = all(torch.equal(t, g[0]) for t in g)
        res["shapes"] = tuple(lay.keys.shape) == (8 // world, 32, 16) and tuple(lay.bias.shape) == (8 // world, 16)
        # ranks seeded ALIKE: the expert shards still differ (generator offset by rank)
        torch.manual_seed(7)
        lay = _make()
        k = [torch.empty_like(lay.keys) for _ in range(world)]
        dist.all_gather(k, lay.keys.detach())
        res["shards_differ"] = all(not torch.equal(k[i], k[j]) for i in range(world) for j in range(i + 1, world))
        res["keys_scale"] = abs(float(lay.keys.std()) - 32 ** -0.5) < 0.05
        # the schedule is the group's first rank's draw everywhere
        torch.manual_seed(200 + rank)
        import random
        random.seed(200 + rank)
        lay2.set_total_steps(0)
        s = lay2.prob_flips_final[0].to(torch.uint8)
        ss = [torch.empty_like(s) for _ in range(world)]
        dist.all_gather(ss, s)
        res["schedule_equal"] = all(torch.equal(t, ss[0]) for t in ss) and s.numel() == 10
        # a rank's slice of a single-GPU competesmoe state dict loads with strict=True
        full = get_moe("competesmoe")(32, 8, 16, n_heads=2, activation=Fn.relu, bias=True, log_interval=None, args=_args())
        sd = full.state_dict()
        El = 8 // world
        mine = {n: (t[rank * El:(rank + 1) * El] if n in ("keys", "values", "bias") else t) for n, t in sd.items()}
        lay.load_state_dict(mine, strict=True)
        res["state_dict"] = torch.equal(lay.keys, full.keys[rank * El:(rank + 1) * El]) and set(lay.state_dict()) == set(sd)
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_competesmoe_ep_constructor_init_and_schedule_gloo(world):
    """Refusals (is_att, fp8 experts, an expert count the ranks do not divide), the replicated gate broadcast from the group's first
    rank, shards that differ under one seed, the schedule equal on every rank, and single-GPU state-dict slices loading strictly."""
    res = _launch(_ctor_worker, world)
    for r in range(world):
        assert res[r] == {"is_att": True, "fp8": True, "divide": True, "w_gate_equal": True, "shapes": True, "shards_differ": True,
                          "keys_scale": True, "schedule_equal": True, "state_dict": True}, (r, res[r])


def _disagree_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        lay = _make().train()
        lay.step_warm, lay.flip_steps = 0, 4
        lay.prob_flips_final = {0: torch.tensor([True, False, True, True])}
        out = {}
        # (1) the competing decision differs: rank 0 is on a competition step, the others are not
        lay.set_current_steps(0 if rank == 0 else 1)
        x = torch.randn(2, 8, 32, requires_grad=True)
        try:
            lay(x, id_layer=0)
            out["decision"] = None
        except RuntimeError as e:
            out["decision"] = str(e)
        # (2) everyone competes, but the token counts differ (the all-gather needs equal sizes)
        lay.set_current_steps(2)
        x = torch.randn(2, 8 + rank, 32, requires_grad=True)
        try:
            lay(x, id_layer=0)
            out["tokens"] = None
        except RuntimeError as e:
            out["tokens"] = str(e)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_competesmoe_ep_rank_disagreement_raises_everywhere_gloo():
    """A disagreement on the competing decision, or on T on a competition step, raises the same error on every rank before any
    collective of the step could hang."""
    res = _launch(_disagree_worker, 2)
    for key in ("decision", "tokens"):
        msgs = [res[r][key] for r in range(2)]
        assert all(m is not None and "disagree" in m for m in msgs), msgs
        assert msgs[0] == msgs[1]
