"""CPU: the MXFP8 weight-gradient entries (csmoe_token_pad_bound, csmoe_quantize_mxfp8_tokens, csmoe_grouped_wgrad_mxfp8) are
exported with ctypes signatures and reject bad arguments before any launch; args.fp8_wgrad needs args.fp8_experts."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 12               # a non-null, 16-byte aligned address that is never dereferenced (validation fails first)


def test_new_entries_are_exported_with_signatures():
    import ctypes
    from competesmoe_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("csmoe_token_pad_bound", "csmoe_quantize_mxfp8_tokens", "csmoe_grouped_wgrad_mxfp8"):
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s


def test_token_pad_bound():
    from competesmoe_amd import _lib, ops
    for n, E in ((0, 1), (1, 1), (128, 1), (129, 1), (1000, 7), (65536, 128)):
        b = _lib.lib.csmoe_token_pad_bound(n, E)
        assert b == ops.token_pad_bound(n, E) == (n + 127 * E + 127) // 128 * 128
        assert b % 128 == 0


def _quant(**kw):
    from competesmoe_amd import _lib
    a = dict(x=FAKE, ldx=64, n=100, C=64, dtype=_lib.BF16, offsets=FAKE, E=4, n_pad=None, poff=FAKE, qt=FAKE, st=FAKE, q=None, s=None)
    a.update(kw)
    if a["n_pad"] is None:
        a["n_pad"] = _lib.lib.csmoe_token_pad_bound(a["n"], a["E"])
    rc = _lib.lib.csmoe_quantize_mxfp8_tokens(a["x"], a["ldx"], a["n"], a["C"], a["dtype"], a["offsets"], a["E"], a["n_pad"], a["poff"],
                                              a["qt"], a["st"], a["q"], a["s"], None)
    return rc, _lib.lib.csmoe_last_error()


def test_token_quantiser_rejects_bad_arguments():
    from competesmoe_amd import _lib
    rc, msg = _quant(dtype=_lib.F32)
    assert rc == 1 and b"dtype" in msg
    rc, msg = _quant(poff=None)
    assert rc == 1 and b"poff" in msg
    rc, msg = _quant(offsets=None)
    assert rc == 1 and b"offsets" in msg
    bound = _lib.lib.csmoe_token_pad_bound(100, 4)
    rc, msg = _quant(n_pad=bound - 128)
    assert rc == 1 and b"n_pad" in msg
    rc, msg = _quant(n_pad=bound + 64)                                # not a multiple of 128
    assert rc == 1 and b"n_pad" in msg
    rc, msg = _quant(q=FAKE)                                          # q without s
    assert rc == 1 and b"row orientation" in msg
    rc, msg = _quant(C=48, ldx=48)                                    # C not a multiple of 32
    assert rc != 0 and b"C % 32" in msg


def _wgrad(**kw):
    from competesmoe_amd import _lib
    a = dict(Aq=FAKE, lda=512, As=FAKE, ldas=16, Bq=FAKE, ldb=512, Bs=FAKE, ldbs=16, poff=FAKE, E=4, n_pad=512, Na=64, Nb=64,
             c_ptrs=FAKE, ldc=64, out_dtype=_lib.F32, accumulate=0, xcd_order=None)
    a.update(kw)
    rc = _lib.lib.csmoe_grouped_wgrad_mxfp8(a["Aq"], a["lda"], a["As"], a["ldas"], a["Bq"], a["ldb"], a["Bs"], a["ldbs"], a["poff"],
                                            a["E"], a["n_pad"], a["Na"], a["Nb"], a["c_ptrs"], a["ldc"], a["out_dtype"], a["accumulate"],
                                            a["xcd_order"], None)
    return rc, _lib.lib.csmoe_last_error()


def test_wgrad_rejects_bad_arguments():
    rc, msg = _wgrad(out_dtype=7)
    assert rc == 1 and b"out_dtype" in msg
    rc, msg = _wgrad(Na=60)
    assert rc == 1 and b"multiples of 8" in msg
    rc, msg = _wgrad(Nb=100, ldc=104)
    assert rc == 1 and b"multiples of 8" in msg
    rc, msg = _wgrad(poff=None)
    assert rc == 1 and b"poff" in msg
    rc, msg = _wgrad(lda=384)                                         # leading dimension below n_pad
    assert rc == 1 and b"n_pad" in msg
    rc, msg = _wgrad(n_pad=500, lda=512, ldb=512)                     # n_pad not a multiple of 128
    assert rc == 1 and b"n_pad" in msg
    rc, msg = _wgrad(c_ptrs=None)
    assert rc == 1 and b"null" in msg


def test_fp8_wgrad_needs_fp8_experts():
    """args.fp8_wgrad without args.fp8_experts is refused; the environment default is read once per process (a fresh child)."""
    code = ("import sys, types, torch.nn.functional as F; sys.path.insert(0, %r)\n"
            "from competesmoe_amd.pretrain import get_moe\n"
            "args = types.SimpleNamespace(balance_loss_coef=0.01, n_shared_experts=2, test_only=False%s)\n"
            "try:\n"
            "    get_moe('deepseekv2')(64, 8, 64, n_heads=2, activation=F.relu, log_interval=None, args=args)\n"
            "    print('built')\n"
            "except ValueError as e:\n"
            "    print('refused', e)\n")
    env = dict(os.environ, CSMOE_FP8_WGRAD="1")
    r = subprocess.run([sys.executable, "-c", code % (ROOT, "")], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert "refused" in r.stdout and "fp8_experts" in r.stdout, (r.stdout, r.stderr)
    env.pop("CSMOE_FP8_WGRAD")
    r = subprocess.run([sys.executable, "-c", code % (ROOT, ", fp8_wgrad=True")], env=env, capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert "refused" in r.stdout, (r.stdout, r.stderr)
    r = subprocess.run([sys.executable, "-c", code % (ROOT, "")], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert "built" in r.stdout, (r.stdout, r.stderr)
