"""CPU tests of the drop-in boundary: libpdae_hip.so loads without a GPU and
exports exactly the entry points include/pdae.h declares; the Python operator
layer refuses to run without a GPU instead of falling back."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "pdae.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pdae_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_path():
    names = _declared()
    for must in ("pdae_furthest_point_sampling", "pdae_knn", "pdae_ball_query", "pdae_group_points",
                 "pdae_gather_points", "pdae_chamfer_forward", "pdae_chamfer_backward",
                 "pdae_emd_approxmatch"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from point_dae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(handle, name), f"{name} declared in pdae.h but not exported"
    assert sorted(_lib.exported_symbols()) == _declared()      # binding covers the whole ABI
    handle.pdae_version.restype = ctypes.c_char_p
    assert handle.pdae_version().startswith(b"pdae-hip gfx950")
    bound = _lib.lib()                                             # every entry is bound as the reader read it
    decls, _ = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert sorted(decls) == _declared()
    for name, (restype, argtypes) in decls.items():
        fn = getattr(bound, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name


_i, _f, _d, _ll, _vp, _sz = (ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p,
                             ctypes.c_size_t)
# one entry per kind of thing the header reader must get right, written out by hand: name -> (restype, argtypes)
PINNED = {
    "pdae_furthest_point_sampling": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "pdae_ball_query": (_i, [_i, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),                    # a float between ints
    "pdae_mean_sum2": (_i, [_ll, _vp, _ll, _vp, _vp, _vp, _vp]),
    "pdae_linsvc_cg_update": (_i, [_i, _i, _i, _d, _d, _i] + [_vp] * 7),                  # doubles between ints
    "pdae_adamw_step_segments": (_i, [_ll, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _i, _vp, _vp]),   # a struct pointer
    "pdae_set_deterministic": (_i, [_vp, _sz]),
    "pdae_pool_bn_backward_workspace": (_ll, [_ll, _i]),                                 # a long long return
    "pdae_rows_wgrad_workspace": (_i, [_i, _i, _vp, _vp, _vp]),                           # a *_workspace that returns int
    "pdae_ctx_current": (_vp, []),
    "pdae_deterministic": (_i, []),
    "pdae_version": (ctypes.c_char_p, []),
    "pdae_last_error": (ctypes.c_char_p, []),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_header_reader_pinned_signatures(name):
    from point_dae_amd import _lib
    decls, _ = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert decls[name] == PINNED[name]


def test_header_reader_type_map_is_closed():
    from point_dae_amd import _lib
    with pytest.raises(ValueError, match="pdae_x"):
        _lib.parse_header("/* a type outside the map */\nint pdae_x(unsigned n);\n")
    with pytest.raises(ValueError, match="pdae_y"):
        _lib.parse_header("unsigned pdae_y(int n);\n")
    decls, const = _lib.parse_header(
        "#define PDAE_N 3   /* pdae_not_declared(int) */\n"
        "int pdae_a(int, const float* /*nullable*/, long long n[], const int32_t counts[2], size_t);  // pdae_nor_this(int)\n"
        "const float* pdae_b(void);\nint64_t pdae_c();\nenum { PDAE_P = 1, PDAE_M = -2 };\n")
    assert decls == {"pdae_a": (_i, [_i, _vp, _vp, _vp, _sz]), "pdae_b": (_vp, []), "pdae_c": (_ll, [])}
    assert const == {"PDAE_N": 3, "PDAE_P": 1, "PDAE_M": -2}


def test_header_constants_and_their_mirrors():
    from point_dae_amd import _lib, affinity_ops, linsvc_ops, svm_ops, vote_ops
    want = {"PDAE_ADAMW_MAX_SEGMENTS": 8, "PDAE_SVM_MAX_PAIR": 2048, "PDAE_SVM_MAX_CLASSES": 64, "PDAE_SVM_MAX_C": 8,
            "PDAE_SVM_PREDICT_MAX_TRAIN": 12288, "PDAE_LINSVC_MAX_CLASSES": 64, "PDAE_LINSVC_SC": 8, "PDAE_LINSVC_FL": 8,
            "PDAE_PROBE_MAX_CLASSES": 64, "PDAE_PROBE_BATCH": 64, "PDAE_VOTE_MAX_CLASSES": 64,
            "PDAE_GEMM_F32MFMA": 0, "PDAE_GEMM_BF16X3": 1, "PDAE_OK": 0, "PDAE_ERR_UNSUPPORTED": -3}
    for name, value in want.items():
        assert _lib.CONST[name] == value, name
    assert set(_lib.CONST) == set(want) | {"PDAE_ERR_BAD_ARG", "PDAE_ERR_LAUNCH"}
    assert (svm_ops.MAX_PAIR, vote_ops.MAX_CLASSES, affinity_ops.BATCH, linsvc_ops.SC, linsvc_ops.FL) == (2048, 64, 64, 8, 8)
    assert (_lib.ADAMW_MAX_SEGMENTS, _lib.GEMM_F32MFMA, _lib.GEMM_BF16X3) == (8, 0, 1)
    assert ctypes.sizeof(_lib.AdamwSegment) == 24                  # pdae_adamw_segment of include/pdae.h
    assert _lib.AdamwSegment._fields_ == [("offset", _ll), ("count", _ll), ("lr", _f), ("weight_decay", _f)]


def test_missing_header_is_reported(tmp_path):
    """The binding reads include/pdae.h relative to itself: a copy of _lib.py without the header beside it says so."""
    import importlib.util
    from point_dae_amd import _lib
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    (pkg / "_lib.py").write_text(open(_lib.__file__).read())
    spec = importlib.util.spec_from_file_location("_lib_without_header", str(pkg / "_lib.py"))
    with pytest.raises(Exception) as err:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(err.value).__name__ == "NativeLibraryMissing" and str(tmp_path / "include" / "pdae.h") in str(err.value)


def test_no_cpu_fallback():
    from point_dae_amd import chamfer_dist, pointnet2_utils
    from point_dae_amd.knn_cuda import KNN
    x = torch.rand(2, 64, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        pointnet2_utils.furthest_point_sample(x, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        chamfer_dist.ChamferDistanceL2()(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        KNN(4, transpose_mode=True)(x, x[:, :3])
    from point_dae_amd import nn_ops, rows
    lin = torch.nn.Linear(8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        nn_ops.mlp_chain(torch.rand(4, 8), [lin, lin])          # the coarse heads: no CPU / framework path either
    with pytest.raises(RuntimeError, match="GPU"):
        rows.linear_any(torch.rand(4, 8), lin.weight, lin.bias)


def test_product_does_not_import_oracle():
    """oracle/ is test infrastructure: nothing under point_dae_amd/ may use it."""
    pkg = os.path.join(ROOT, "point_dae_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "pdae_oracle" not in src or f.endswith((".hip", ".h", ".cpp")) , f


def test_product_has_no_library_gemm_call_sites():
    """Every dense layer of the product models runs on the hand-written kernels: no F.linear / torch.mm /
    matmul / bmm / addmm call on device tensors in the package (host-side 3x3 composition of the drawn affine
    maps in corrupt_util_tensor.py / datasets.py / synthetic.py is numpy or CPU torch)."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'point_dae_amd')
    host_side = {'corrupt_util_tensor.py', 'datasets.py', 'synthetic.py', 'svm_probe.py'}
    pat = re.compile(r'F\.linear\(|torch\.(mm|bmm|addmm|matmul|einsum)\(|\.matmul\(|F\.conv1d\(|F\.conv2d\(')
    hits = []
    for name in sorted(os.listdir(root)):
        if name.endswith('.py') and name not in host_side:
            for i, line in enumerate(open(os.path.join(root, name)), 1):
                code = line.split('#')[0]
                if pat.search(code) or re.search(r'[\w\)\]] @ [\w\(]', code):
                    hits.append('%s:%d %s' % (name, i, line.strip()))
    assert not hits, hits


def test_library_is_built_without_slp_packed_fp32():
    """csrc/Makefile keeps `-fno-slp-vectorize`: hipcc's SLP vectoriser packs scalar fp32 accumulations into
    v_pk_{fma,mul,add}_f32 with operand selects, which gfx950 computes wrongly (low halves, lanes 16-31) while another
    wave of the CU runs bf16 MFMAs beside ds_read_b128 -- another stream or another process (tools/xproc_repro.hip,
    INTEGRATION.md).  __graft_entry__.build() must not override the flags either."""
    with open(os.path.join(ROOT, 'point_dae_amd', 'csrc', 'Makefile')) as f:
        flags = [ln for ln in f if ln.startswith('FLAGS')]
    assert flags and '-fno-slp-vectorize' in flags[0] and '-ffp-contract=off' in flags[0], flags
    with open(os.path.join(ROOT, '__graft_entry__.py')) as f:
        assert 'FLAGS=' not in f.read()
