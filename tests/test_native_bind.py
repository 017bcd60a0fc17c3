"""CPU: transoar_amd._native binds every library from its public header -- the parser reads every prototype under include/,
maps each C type the headers use to its ctypes type and refuses any other, and bind() fails loudly on a missing library, a
stale ABI or a symbol the library does not export.  No kernel is launched."""
import ctypes
import os
import re

import pytest

from transoar_amd import _native
from transoar_amd._native import NativeLibraryError, bind, parse_header

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = sorted(f for f in os.listdir(INCLUDE) if re.match(r"transoar_[a-z0-9]+\.h$", f))
P, I, L, U, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_uint, ctypes.c_size_t
F, D = ctypes.c_float, ctypes.c_double


def _protos(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return parse_header(f.read(), header)


@pytest.mark.parametrize("header", HEADERS)
def test_parser_reads_every_prototype(header):
    """The names the parser returns are the names test_abi's regex finds: no prototype is skipped."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    declared = set(re.findall(r"\b(transoar_[a-z_0-9]+)\s*\(", text))
    assert declared and set(_protos(header)) == declared


def test_every_type_of_the_headers_once():
    msda, attn, conv = _protos("transoar_msda3d.h"), _protos("transoar_attn.h"), _protos("transoar_convgemm.h")
    assert msda["transoar_msda3d_forward_fused"] == (I, [P, P, P, L, P] + [I] * 7 + [P, P])            # long in slot 4
    assert attn["transoar_roi_attn_forward"] == (I, [P] * 8 + [Z, I, I, I, L, I, I, P])               # size_t and long
    assert _protos("transoar_optim.h")["transoar_adamw_step"] == (I, [P, P, P, I, D, D, F, F, P])     # a struct pointer too
    assert msda["transoar_msda3d_forward"] == (I, [P] * 6 + [I] * 9 + [P, U, P])                      # unsigned flags
    assert msda["transoar_msda3d_strerror"] == (ctypes.c_char_p, [I])
    assert msda["transoar_msda3d_profile_enable"] == (None, [I])
    assert conv["transoar_conv3d_wgrad_part_floats"] == (L, [I] * 4)
    assert msda["transoar_msda3d_backward_workspace_bytes"] == (Z, [I] * 9 + [U])
    assert msda["transoar_msda3d_plan"] == (I, [I] * 9 + [P, U, I, P])                                 # host pointers in and out
    assert msda["transoar_msda3d_abi_version"] == (I, [])
    # and they are what the loaded library carries
    fused = _native.lib.transoar_msda3d_forward_fused
    assert (fused.restype, fused.argtypes) == msda["transoar_msda3d_forward_fused"]
    assert _native.lib.transoar_msda3d_abi_version.argtypes == []


@pytest.mark.parametrize("proto", ["int transoar_x(short n);", "int transoar_x(unsigned int n);", "short transoar_x(void);",
                                   "void* transoar_x(void);", "int transoar_x(int64_t n);"])
def test_a_type_outside_the_table_is_refused(proto):
    with pytest.raises(NativeLibraryError, match="transoar_x"):
        parse_header(proto, "probe.h")


def test_a_prototype_the_parser_cannot_read_is_an_error():
    with pytest.raises(NativeLibraryError, match="probe.h"):
        parse_header("int transoar_x(int (*callback)(int));", "probe.h")


def test_load_errors(tmp_path):
    with pytest.raises(NativeLibraryError, match="_build.py"):
        bind("nosuchlibrary")
    with pytest.raises(NativeLibraryError, match="rebuild"):
        bind("tokens", abi=6)
    with pytest.raises(NativeLibraryError, match="header"):
        bind("tokens", header=str(tmp_path / "missing.h"))
    extra = tmp_path / "transoar_tokens.h"
    extra.write_text(open(os.path.join(INCLUDE, "transoar_tokens.h")).read() + "\nint transoar_tokens_not_there(int n);\n")
    with pytest.raises(NativeLibraryError, match="transoar_tokens_not_there"):
        bind("tokens", abi=7, header=str(extra))
    assert bind("tokens", abi=7).transoar_tokens_abi_version() == 7
