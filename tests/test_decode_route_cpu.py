"""CPU: the host side of the decode front end (csmoe_decode_route): its shape rule, its argument validation before any launch, the
identity rules under which the route plan is handed out, the switch, and the torch reference of the bins."""
import torch

from tests.decode_route_ref import ref_bins


def test_decode_route_shape_rule():
    from competesmoe_amd import _lib
    L, bf16 = _lib.lib, _lib.BF16
    assert L.csmoe_decode_route_ok(1, 4096, 256, 2, bf16, 0) == 1
    assert L.csmoe_decode_route_ok(512, 128, 8, 2, bf16, 0) == 1
    assert L.csmoe_decode_route_ok(512, 128, 8, 2, bf16, 1) == 1
    assert L.csmoe_decode_route_ok(513, 128, 8, 2, bf16, 0) == 0          # n = 1026 routed rows
    assert L.csmoe_decode_route_ok(1, 128, 257, 2, bf16, 0) == 0          # E = 257
    assert L.csmoe_decode_route_ok(1, 132, 8, 2, bf16, 0) == 0            # D = 132: not a multiple of 8
    assert L.csmoe_decode_route_ok(1, 128, 8, 2, _lib.F32, 0) == 0        # fp32
    assert L.csmoe_decode_route_ok(1, 128, 4, 5, bf16, 0) == 0            # K > E
    assert L.csmoe_decode_route_ok(0, 128, 8, 2, bf16, 0) == 0            # 1 <= T
    assert L.csmoe_decode_route_ok(1, 136, 8, 2, bf16, 0) == 1            # D % 8 == 0 is enough without the quantised rows ...
    assert L.csmoe_decode_route_ok(1, 136, 8, 2, bf16, 1) == 0            # ... with them D % 32 == 0
    assert L.csmoe_decode_route_workspace_bytes(1) % 16 == 0
    assert L.csmoe_decode_route_workspace_bytes(1024) >= 4 * (1 + 64)     # one counter per 16-row block and the call's own


def test_decode_route_validates_before_any_launch():
    from competesmoe_amd import _lib
    L, bf16 = _lib.lib, _lib.BF16
    none12 = [None] * 12
    rc = L.csmoe_decode_route(None, None, 8, 64, 4, 9, 0, 0, 1.0, bf16, *none12)
    assert rc == 1 and b"decode_route" in L.csmoe_last_error()            # K > E
    rc = L.csmoe_decode_route(None, None, 8, 64, 4, 2, 9, 0, 1.0, bf16, *none12)
    assert rc == 1 and b"mode" in L.csmoe_last_error()
    # a quantised output (xq / xs given; never dereferenced) with D % 32 != 0: unsupported, decided on the shape alone
    rc = L.csmoe_decode_route(None, None, 8, 136, 8, 2, 0, 0, 1.0, bf16, None, None, None, None, None, None, None, None, 16, 16, None, None)
    assert rc == 3 and b"decode_route" in L.csmoe_last_error()
    rc = L.csmoe_decode_route(None, None, 8, 128, 8, 2, 0, 0, 1.0, bf16, None, None, None, None, None, None, None, None, 16, None, None, None)
    assert rc == 1 and b"xq and xs" in L.csmoe_last_error()
    rc = L.csmoe_decode_route(None, None, 600, 128, 8, 2, 0, 0, 1.0, bf16, *none12)
    assert rc == 3                                                        # 1200 routed rows
    rc = L.csmoe_decode_route(None, None, 8, 128, 8, 2, 0, 0, 1.0, bf16, *none12)
    assert rc == 1 and b"null" in L.csmoe_last_error()                    # a shape it takes: now the operands are looked at
    assert L.csmoe_decode_route(None, None, 0, 128, 8, 2, 0, 0, 1.0, bf16, *none12) == 0


def test_route_plan_is_only_handed_out_for_the_tensors_it_was_built_from():
    """ops._route_plan_for / ops._quant_rows_for: the rules of ops._route_hist_for (same storage, same numel / shape, same version
    counter), so ops.bin_tokens and ops.quantize_mxfp8 reuse the front end's results for its very idx / x2 and nothing else."""
    from competesmoe_amd import ops
    idx = torch.zeros(128, 2, dtype=torch.int32)
    bins = ops.Bins(None, None, None, None, 256, 8, 2)
    x2 = torch.zeros(128, 64, dtype=torch.bfloat16)
    q = (torch.zeros(128, 64, dtype=torch.uint8), torch.zeros(128, 2, dtype=torch.uint8))
    old = ops._ROUTE_PLAN
    try:
        ops._ROUTE_PLAN = (idx, idx._version, bins, x2, x2._version, q)
        assert ops._route_plan_for(idx, 8) is bins
        assert ops._route_plan_for(idx.view(2, 64, 2).view(128, 2), 8) is bins            # a view of the same ids
        assert ops._route_plan_for(idx.clone(), 8) is None                                # other storage
        assert ops._route_plan_for(idx, 16) is None                                       # other expert count
        assert ops._route_plan_for(idx[:64], 8) is None                                   # other length
        assert ops._quant_rows_for(x2) is q
        assert ops._quant_rows_for(x2.view(2, 64, 64).view(128, 64)) is q                 # a view of the same rows
        assert ops._quant_rows_for(x2.clone()) is None
        assert ops._quant_rows_for(x2.view(64, 128)) is None                              # other shape
        assert ops._quant_rows_for(x2.view(2, 64, 64)) is None                            # not 2-D
        assert ops._quant_rows_for(x2[:64]) is None
        assert ops._quant_rows_for(x2.view(torch.float16)) is None                        # other dtype
        x2[0, 0] = 1                                                                      # edited in place
        assert ops._quant_rows_for(x2) is None
        assert ops._route_plan_for(idx, 8) is bins                                        # the ids were not
        idx[0, 0] = 3
        assert ops._route_plan_for(idx, 8) is None
        ops._ROUTE_PLAN = (idx, idx._version, bins, None, 0, None)                        # a plan without quantised rows
        assert ops._route_plan_for(idx, 8) is bins and ops._quant_rows_for(x2) is None
    finally:
        ops._ROUTE_PLAN = old


def test_decode_front_switch_defaults_off_and_round_trips():
    import os
    import competesmoe_amd
    from competesmoe_amd import ops
    if os.environ.get("CSMOE_DECODE_FRONT") is None:
        assert competesmoe_amd.decode_front() is False
    before = competesmoe_amd.decode_front()
    try:
        assert competesmoe_amd.decode_front(True) is True and ops.decode_front() is True
        assert competesmoe_amd.decode_front() is True
        assert competesmoe_amd.decode_front(False) is False and ops.decode_front() is False
        # off: the layers' test says no whatever the operands are (and without looking at them)
        assert ops.decode_front_applies(None, None, 2, False) is False
    finally:
        competesmoe_amd.decode_front(before)


def test_reference_bins_on_a_hand_written_case():
    idx = torch.tensor([[2, 0], [1, 2], [0, 2]], dtype=torch.int32)       # flat: 2 0 1 2 0 2
    counts, offsets, perm, slot_of = ref_bins(idx, 4)
    assert counts.tolist() == [2, 1, 3, 0]
    assert offsets.tolist() == [0, 2, 3, 6, 6]
    assert perm.tolist() == [1, 4, 2, 0, 3, 5]                            # expert 0: flats 1, 4; expert 1: 2; expert 2: 0, 3, 5
    assert slot_of.tolist() == [3, 0, 2, 4, 1, 5]
    # ids outside [0, E) are skipped
    counts, offsets, perm, slot_of = ref_bins(torch.tensor([[1, 7], [-1, 0]], dtype=torch.int32), 2)
    assert counts.tolist() == [1, 1] and offsets.tolist() == [0, 1, 2]
    assert perm.tolist()[:2] == [3, 0] and slot_of.tolist() == [1, -1, -1, 0]
