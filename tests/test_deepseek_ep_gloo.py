"""CPU (gloo): the constructor, init, state-dict and gradient-hook contract of the pretrain `deepseekv2_ep` / `deepseekv3_ep` layers
(competesmoe_amd/pretrain/deepseek_ep.py).  Their forward / backward against the single-GPU layers: tests/test_deepseek_ep_gpu.py."""
import os
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

NAMES = ("deepseekv2_ep", "deepseekv3_ep")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _args(**kw):
    a = dict(balance_loss_coef=0.01, n_shared_experts=1, test_only=False)
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


def _make(name, D=32, E=8, F=16, bias=True, args=None, **kw):
    import torch.nn.functional as Fn
    from competesmoe_amd.pretrain import get_moe
    return get_moe(name)(D, E, F, n_heads=2, activation=Fn.relu, bias=bias, log_interval=None, args=args or _args(), **kw)


def test_deepseek_ep_layers_are_registered_and_exported():
    import competesmoe_amd.pretrain as P
    assert P.get_moe("deepseekv2_ep") is P.EPDeepSeekV2 and P.get_moe("deepseekv3_ep") is P.EPDeepSeekV3
    assert "EPDeepSeekV2" in P.__all__ and "EPDeepSeekV3" in P.__all__
    assert issubclass(P.EPDeepSeekV2, P.DeepSeekV2) and issubclass(P.EPDeepSeekV3, P.DeepSeekV3)


@pytest.mark.parametrize("name", NAMES)
def test_deepseek_ep_needs_a_process_group(name):
    with pytest.raises(RuntimeError, match="process group"):
        _make(name)


def _ctor_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        import torch.nn.functional as Fn
        from competesmoe_amd.pretrain import get_moe
        out = {}
        for name in NAMES:
            res = {}
            for what, kw in (("is_att", dict(is_att=True, inp_expert=32, out_expert=32)), ("divide", dict(n_experts=9)),
                             ("fp8_wgrad", dict(args=_args(fp8_experts=True, fp8_wgrad=True)))):
                a = dict(dmodel=32, n_experts=8, expert_size=16, n_heads=2, activation=Fn.relu, args=_args())
                a.update(kw)
                try:
                    get_moe(name)(**a)
                    res[what] = False
                except ValueError:
                    res[what] = True
            lay8 = _make(name, args=_args(fp8_experts=True, fp8_weight_cache=True))
            res["fp8_builds"] = lay8.fp8_experts and lay8.fp8_weight_cache
            # shapes: the routed shard, the shared tensors in full for one and two shared experts
            El = 8 // world
            ok = True
            for ns in (1, 2):
                lay = _make(name, args=_args(n_shared_experts=ns))
                ok = ok and tuple(lay.keys.shape) == (El, 32, 16) and tuple(lay.values.shape) == (El, 16, 32)
                ok = ok and tuple(lay.bias.shape) == (El, 16) and tuple(lay.w_gate.shape) == (8, 32) and lay.n_experts == 8
                ok = ok and tuple(lay.keys_shared.shape) == (1, 32, 16 * ns) and tuple(lay.values_shared.shape) == (1, 16 * ns, 32)
                ok = ok and tuple(lay.bias_shared.shape) == (1, 16 * ns)
            res["shapes"] = ok
            res["no_bias"] = _make(name, bias=False).bias_shared is None
            # ranks seeded DIFFERENTLY: the replicated tensors still agree -- broadcast from the group's first rank
            torch.manual_seed(100 + rank)
            lay = _make(name)
            eq = True
            for nme in ("w_gate", "o_bias", "keys_shared", "values_shared", "bias_shared"):
                t = getattr(lay, nme).detach()
                g = [torch.empty_like(t) for _ in range(world)]
                dist.all_gather(g, t)
                eq = eq and all(torch.equal(v, g[0]) for v in g)
            res["replicated_equal"] = eq
            res["shared_drawn"] = float(lay.keys_shared.std()) > 0 and float(lay.values_shared.std()) > 0
            # ranks seeded ALIKE: the expert shards still differ (generator offset by rank)
            torch.manual_seed(7)
            lay = _make(name)
            k = [torch.empty_like(lay.keys) for _ in range(world)]
            dist.all_gather(k, lay.keys.detach())
            res["shards_differ"] = all(not torch.equal(k[i], k[j]) for i in range(world) for j in range(i + 1, world))
            res["keys_scale"] = abs(float(lay.keys.std()) - 32 ** -0.5) < 0.05
            # a rank's slice of the single-GPU layer's state dict loads with strict=True
            full = _make(name[:-3])
            sd = full.state_dict()
            mine = {n: (t[rank * El:(rank + 1) * El] if n in ("keys", "values", "bias") else t) for n, t in sd.items()}
            lay.load_state_dict(mine, strict=True)
            res["state_dict"] = (torch.equal(lay.keys, full.keys[rank * El:(rank + 1) * El]) and set(lay.state_dict()) == set(sd)
                                 and torch.equal(lay.keys_shared, full.keys_shared))
            out[name] = res
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_deepseek_ep_constructor_init_and_state_dict_gloo(world):
    """Refusals (is_att, an expert count the ranks do not divide, fp8_wgrad), fp8 experts accepted, shard and shared shapes, the
    replicated tensors broadcast from the group's first rank, shards that differ under one seed, strict state-dict slices."""
    res = _launch(_ctor_worker, world)
    for r in range(world):
        for name in NAMES:
            assert res[r][name] == {"is_att": True, "divide": True, "fp8_wgrad": True, "fp8_builds": True, "shapes": True, "no_bias": True,
                                    "replicated_equal": True, "shared_drawn": True, "shards_differ": True, "keys_scale": True,
                                    "state_dict": True}, (r, name, res[r][name])


def _hook_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        out = {}
        for name in NAMES:
            lay = _make(name)
            ok = True
            for nme in ("keys_shared", "values_shared", "bias_shared"):
                p = getattr(lay, nme)
                for _ in range(2):                                   # two micro-batches, no zeroing in between
                    (p * (rank + 1)).sum().backward()
                want = 2.0 * sum(r + 1 for r in range(world))
                ok = ok and torch.equal(p.grad, torch.full_like(p, want))
            out[name] = ok
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_replicated_shared_expert_gradients_with_two_micro_batches_gloo(world):
    """The shared expert's gradients are summed over the group once per backward pass: after two passes without zeroing, every rank
    holds 2 * sum_r (r + 1) (a hook that reduced the accumulated .grad would count the first pass twice)."""
    res = _launch(_hook_worker, world)
    for r in range(world):
        assert res[r] == {n: True for n in NAMES}, (r, res[r])


def test_smoe_ep_and_competesmoe_ep_share_the_broadcast_helpers():
    from competesmoe_amd.pretrain import competesmoe_ep, deepseek_ep, smoe_ep
    assert competesmoe_ep._broadcast is smoe_ep._broadcast is deepseek_ep._broadcast
