"""CPU: the one-pass gather + MXFP8 quantiser entries (csmoe_dispatch_rows_mxfp8, csmoe_dispatch_tokens_mxfp8) are exported with
ctypes signatures and reject bad arguments before any launch; their bytes on the GPU: tests/test_dispatch_quant_gpu.py."""
import pytest

FAKE = 1 << 12               # a non-null, 16-byte aligned address that is never dereferenced (validation fails first)
ENTRIES = ("csmoe_dispatch_rows_mxfp8", "csmoe_dispatch_tokens_mxfp8")


def test_new_entries_are_exported_with_signatures():
    import ctypes
    from competesmoe_amd import _lib, ops
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ENTRIES:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert callable(ops.dispatch_rows_mxfp8) and callable(ops.dispatch_tokens_mxfp8)


def _call(entry, **kw):
    from competesmoe_amd import _lib
    a = dict(x=FAKE, index=FAKE, K=2, xs=FAKE, q=FAKE, s=FAKE, n=100, D=64, dtype=_lib.BF16)
    a.update(kw)
    rc = getattr(_lib.lib, entry)(a["x"], a["index"], a["K"], a["xs"], a["q"], a["s"], a["n"], a["D"], a["dtype"], None)
    return rc, _lib.lib.csmoe_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_arguments_are_refused_before_any_launch(entry):
    from competesmoe_amd import _lib
    rc, msg = _call(entry, dtype=_lib.F32)
    assert rc == 1 and b"dtype" in msg and entry[6:].encode() in msg
    rc, msg = _call(entry, D=48)
    assert rc == 1 and b"D % 32" in msg
    rc, msg = _call(entry, D=0)
    assert rc == 1
    rc, msg = _call(entry, q=None)
    assert rc == 1 and b"null q / s" in msg
    rc, msg = _call(entry, s=None)
    assert rc == 1 and b"null q / s" in msg
    rc, msg = _call(entry, index=None)
    assert rc == 1 and b"index" in msg
    rc, msg = _call(entry, x=None)
    assert rc == 1 and b"null x" in msg
    rc, msg = _call(entry, K=0)
    assert rc == 1 and b"K=0" in msg
    rc, msg = _call(entry, x=FAKE + 2)
    assert rc == 1 and b"aligned" in msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_rows_is_a_no_op(entry):
    assert _call(entry, n=0)[0] == 0
    assert _call(entry, n=0, x=None, index=None, xs=None, q=None, s=None)[0] == 0
    from competesmoe_amd import _lib
    assert _call(entry, n=0, dtype=_lib.F32)[0] == 1          # the dtype is checked even then
