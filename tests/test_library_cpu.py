"""CPU-side checks of the C-ABI: the library builds (hipcc cross-compiles without a GPU), loads,
and exports every symbol include/ofd.h declares; the ctypes table binds exactly that set."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def libpath():
    from opticalflowdiffusion_amd import build
    return build.build(verbose=False)


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "ofd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ofd_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(libpath):
    lib = ctypes.CDLL(libpath)
    names = declared_symbols()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in include/ofd.h but not exported: {missing}"


def test_ctypes_table_matches_header(libpath):
    from opticalflowdiffusion_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    L = _lib.lib()
    assert L.ofd_version() >= 1
    assert L.ofd_last_error() is not None


def test_argument_errors_without_gpu(libpath):
    """argument validation happens before any HIP call: usable (and tested) on a CPU-only host"""
    from opticalflowdiffusion_amd import _lib
    L = _lib.lib()
    assert L.ofd_splat_workspace_bytes(2, 8, 8) == 16 + 2 * 256 * 4 + 8 * 2 * 8 * 8
    rc = L.ofd_splat_fwd(None, None, None, 1, 1, 8, 8, 3, 0, 0, 4, None, 0, None)      # null pointers
    assert rc == -1 and b"null" in L.ofd_last_error()
    rc = L.ofd_splat_fwd(None, None, None, 1, 1, 8, 8, 16, 0, 0, 4, None, 0, None)     # H // scale == 0
    assert rc == -1 and b"scale" in L.ofd_last_error()
    rc = L.ofd_warp_holes(None, None, 1, 1, 4, 4, 7, 1, None)
    assert rc == -1
    args = _lib.ConvArgs()
    assert L.ofd_conv_forward(ctypes.byref(args), None) == -1
    assert L.ofd_conv_gn_partial_count(2, 16, 64, 64) == 2 * 2 * 2 * 4 * 8 * 2
    assert L.ofd_conv_weight_elems(64, 16, 7) == 49 * 16 * 64
    # the fused LinearAttention entry points: one null-pointer call and one bad-C call each (p: a real, 16-byte aligned host address --
    # validation returns before anything could read it)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    calls = {
        "la_weight_prep": lambda a, C: L.ofd_la_weight_prep(a, p, p, p, p, p, C, None),
        "linear_attention_block": lambda a, C: L.ofd_linear_attention_block(a, *[p] * 8, 1, 4, C, 1e-5, 1e-3, None),
        "linear_attention_block_train": lambda a, C: L.ofd_linear_attention_block_train(a, *[p] * 14, 1, 4, C, 1e-5, 1e-3, None),
        "linear_attention_core_proj": lambda a, C: L.ofd_linear_attention_core_proj(a, *[p] * 7, C, 1, 4, None),
        "linear_attention_block_backward": lambda a, C: L.ofd_linear_attention_block_backward(a, *[p] * 13, C, 1, 4, None),
        "layernorm_c_backward_residual": lambda a, C: L.ofd_layernorm_c_backward_residual(a, p, p, None, p, p, 4, C, 1e-5, 0, None),
    }
    good_c = {"linear_attention_core_proj": 128}
    for name, call in calls.items():
        assert call(None, good_c.get(name, 64)) == -1 and b"null" in L.ofd_last_error() and name.encode() in L.ofd_last_error(), name
        assert call(p, 96) == -1 and b"C=96" in L.ofd_last_error() and name.encode() in L.ofd_last_error(), name
    # widths the other forms take but these do not, sizes, alignment
    assert calls["linear_attention_block_train"](p, 128) == -1 and calls["linear_attention_block_backward"](p, 128) == -1
    assert calls["linear_attention_core_proj"](p, 64) == -1
    assert L.ofd_linear_attention_block(*[p] * 9, 0, 4, 64, 1e-5, 1e-3, None) == -1 and b"B=0" in L.ofd_last_error()
    assert L.ofd_linear_attention_block(*[p] * 9, 1, 0, 64, 1e-5, 1e-3, None) == -1 and b"n=0" in L.ofd_last_error()
    odd = ctypes.c_void_p(p.value + 2)
    assert L.ofd_linear_attention_block(odd, *[p] * 8, 1, 4, 64, 1e-5, 1e-3, None) == -1 and b"aligned" in L.ofd_last_error()
    assert L.ofd_linear_attention_block(p, odd, *[p] * 7, 1, 4, 64, 1e-5, 1e-3, None) == -1 and b"aligned" in L.ofd_last_error()
    assert L.ofd_version() >= 4                                            # the minor went up with the new symbols
    # the weight-gradient entry points that take a bias accumulator: it is not optional there
    assert L.ofd_conv_wgrad_bias(ctypes.byref(args), p, p, None, None) == -1 and b"conv_wgrad_bias: null" in L.ofd_last_error()
    assert L.ofd_conv7_wgrad_bias(p, p, p, None, 1, 8, 32, 8, None) == -1 and b"conv7_wgrad_bias: null" in L.ofd_last_error()
    assert L.ofd_conv7_wgrad_bias(p, p, p, p, 1, 8, 32, 24, None) == -1 and b"packed to 24 channels" in L.ofd_last_error()
    assert L.ofd_version() >= 7


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from opticalflowdiffusion_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.OfdError, match="no CPU or PyTorch fallback"):
        _lib.lib()
