"""The binding of the PAPER id pass's interface (DR_OPT_DEVICE_IDS, dr_last_ids_form): the
header, the ctypes table and the Engine veneer name the same things.  No device needed."""
import os
import re

from dag_rider_amd import _lib as L
from dag_rider_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_constant_matches_header():
    assert L.DR_OPT_DEVICE_IDS == 9
    with open(os.path.join(ROOT, "include", "dagrider_gpu.h")) as f:
        hdr = f.read()
    assert re.search(r"\bDR_OPT_DEVICE_IDS\s*=\s*9\b", hdr)
    assert re.search(r"\bint\s+dr_last_ids_form\s*\(\s*const\s+dr_ctx\s*\*", hdr)
    assert re.search(r"#define\s+DR_ABI_VERSION\s+2\b", hdr)  # additive: the ABI version stays


def test_getter_declared_and_exported():
    assert "dr_last_ids_form" in L.SIGNATURES
    res, args = L.SIGNATURES["dr_last_ids_form"]
    assert res is L.C.c_int and args == [L.P]
    lib = L.lib()  # binds every declared symbol: a missing export raises here
    assert lib.dr_last_ids_form(None) == -1  # no context: nothing requested ids


def test_engine_methods():
    assert callable(getattr(Engine, "set_device_ids", None))
    assert callable(getattr(Engine, "last_ids_form", None))
