"""ctypes binding of libpdae_hip.so -- the C ABI declared in include/pdae.h.

This is the only place the product talks to native code.  There is no CPU
fallback: if the library is missing, or a tensor is not a contiguous float32
(int32 / int64 where the ABI says so) tensor on a HIP device, the call raises.

include/pdae.h is the only place a signature or a constant of the ABI is written: parse_header() reads the
declarations and the integer constants out of its text, once at import, and lib() binds every entry from them.  A new
entry point needs its declaration in the header and nothing here.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDAE_LIB") or os.path.join(_HERE, "libpdae_hip.so")     # PDAE_LIB: another build of the library (A/B runs, tools/lab/ab.sh)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pdae.h")

# the header's value types; every pointer and array parameter is a c_void_p.  Closed: anything else raises.
_CTYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'long long': ctypes.c_longlong, 'int64_t': ctypes.c_longlong,
           'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
           'pdae_stream_t': ctypes.c_void_p, 'pdae_ctx_t': ctypes.c_void_p}


class NativeLibraryMissing(RuntimeError):
    pass


def _ctype(decl, name, ret=False):
    """ctypes type of one parameter (its name may be absent) or, with `ret`, of a return type."""
    words = re.sub(r'\bconst\b', ' ', decl).split()
    if '*' in decl or decl.rstrip().endswith(']'):
        return ctypes.c_char_p if ret and ''.join(words) == 'char*' else ctypes.c_void_p
    for n in (len(words), len(words) - (not ret)):      # all words are the type, or the last is a parameter's name
        if ' '.join(words[:n]) in _CTYPES:
            return _CTYPES[' '.join(words[:n])]
    raise ValueError(f"{name}: type of '{decl.strip()}' is outside the ABI's type map")


def parse_header(text):
    """(decls, const) of a header's text: decls = {name: (restype, argtypes)} of every
    `ret pdae_name(params);`, const = {PDAE_X: int} of the `#define PDAE_X <int>` lines and the enum items."""
    text = re.sub(r'//[^\n]*', ' ', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    const = {k: int(v) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(PDAE_\w+)[ \t]+(-?\d+)[ \t]*$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    const.update((k, int(v)) for k, v in re.findall(r'\b(PDAE_\w+)\s*=\s*(-?\d+)', text))
    decls = {}
    for ret, name, params in re.findall(r'([\w\s*]+?)\b(pdae_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text):
        params = [] if params.strip() in ('', 'void') else params.split(',')
        decls[name] = (_ctype(ret, name, ret=True), [_ctype(p, name) for p in params])
    return decls, const


if not os.path.exists(HEADER_PATH):
    raise NativeLibraryMissing(f"{HEADER_PATH} not found: the binding reads the C ABI from the tree's include/pdae.h")
with open(HEADER_PATH) as _f:
    _DECLS, CONST = parse_header(_f.read())

_lib = None


def exported_symbols():
    """Every symbol include/pdae.h declares (used by the CPU-side ABI test)."""
    return list(_DECLS)


def lib():
    """Load libpdae_hip.so (built by __graft_entry__.build / csrc/Makefile) and bind every entry include/pdae.h declares."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). point_dae_amd has no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _DECLS.items():
            fn = getattr(handle, name)
            fn.argtypes, fn.restype = argtypes, restype
        _lib = handle
    return _lib


_det_ws = None


def set_deterministic(on=True, megabytes=64):
    """Register (or drop) the workspace of include/pdae.h's deterministic mode on the current
    device.  `PDAE_DETERMINISTIC=1` in the environment does this at the first kernel call."""
    global _det_ws
    handle = lib()
    if on:
        _det_ws = torch.empty(megabytes << 20, dtype=torch.uint8, device='cuda')
        _check(handle, 'pdae_set_deterministic', handle.pdae_set_deterministic(_det_ws.data_ptr(), _det_ws.numel()))
    else:
        torch.cuda.synchronize()
        _check(handle, 'pdae_set_deterministic', handle.pdae_set_deterministic(None, 0))
        _det_ws = None


def deterministic():
    return bool(lib().pdae_deterministic())


_def_ws = None


def deferred_begin(megabytes=64):
    """Park the LayerNorm parameter-gradient partials until deferred_flush (include/pdae.h)."""
    global _def_ws
    if _def_ws is None or _def_ws.numel() != megabytes << 20:
        _def_ws = torch.empty(megabytes << 20, dtype=torch.uint8, device='cuda')
    handle = lib()
    _check(handle, 'pdae_deferred_begin', handle.pdae_deferred_begin(_def_ws.data_ptr(), _def_ws.numel()))
    global _def_keep
    _def_keep = []


_def_keep = None      # while reductions are parked: the workspaces their partials live in


def deferred_flush(on):
    global _def_keep
    call('pdae_deferred_flush', on)
    _def_keep = None      # (the flush is enqueued: later allocations reuse the memory behind it in stream order)


_env_checked = False


def _env_mode():
    global _env_checked
    _env_checked = True
    if os.environ.get('PDAE_DETERMINISTIC', '0') not in ('', '0') and _det_ws is None:
        set_deterministic(True, int(os.environ.get('PDAE_DETERMINISTIC_MB', '64')))


def stream_ptr():
    """hipStream_t of torch's current stream on the current device."""
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None else None


def ptr_array(tensors):
    """HOST array of the tensors' device pointers (None: NULL)."""
    return (ctypes.c_void_p * len(tensors))(*[ptr(t) for t in tensors])


def int_array(values):
    return (ctypes.c_int * len(values))(*values)


def require(t, name, dtype=torch.float32, dim=None):
    """Input validation of the reference's CHECK_CUDA / CHECK_CONTIGUOUS /
    CHECK_IS_FLOAT / CHECK_IS_INT macros (extensions/pointnet2/_ext_src/include/
    utils.h:8-28), raised as RuntimeError like AT_ASSERT does."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on the GPU (CPU not supported)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be a {dtype} tensor, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")
    if dim is not None and t.dim() != dim:
        raise RuntimeError(f"{name} must have {dim} dimensions, got {t.dim()}")
    return t


CALL_HOOK = None      # tools / tests: callable(name, args) seen by every C entry call (e.g. tools/dump_gemm_shapes.py)


def call(name, on, *args):
    """Invoke one C entry on torch's current stream of `on`'s device; raise on a
    non-zero status."""
    handle = lib()
    if CALL_HOOK is not None:
        CALL_HOOK(name, args)
    if not _env_checked:
        _env_mode()
    if on.device.index != torch.cuda.current_device():
        with torch.cuda.device(on.device):
            rc = getattr(handle, name)(*args, stream_ptr())
    else:
        rc = getattr(handle, name)(*args, stream_ptr())
    if rc != 0:
        msg = handle.pdae_last_error().decode()
        raise RuntimeError(f"{name} failed with status {rc}: {msg}")


def _check(handle, name, rc):
    if rc != 0:
        raise RuntimeError(f"{name} failed with status {rc}: {handle.pdae_last_error().decode()}")


class Context:
    """A library context (include/pdae.h pdae_ctx_*): the deterministic-mode workspace, the parked reductions and the
    GEMM arithmetic of the host thread that makes it current.  `with Context():` works on a private context."""

    def __init__(self):
        h = ctypes.c_void_p()
        _check(lib(), 'pdae_ctx_create', lib().pdae_ctx_create(ctypes.byref(h)))
        self.handle, self._prev, self._keep = h, None, []

    def __enter__(self):
        self._prev = lib().pdae_ctx_current()
        lib().pdae_ctx_set_current(self.handle)
        return self

    def set_deterministic(self, megabytes=64):
        """Deterministic mode for THIS context (it must be current): the workspace belongs to the context."""
        ws = torch.empty(megabytes << 20, dtype=torch.uint8, device='cuda')
        self._keep.append(ws)
        _check(lib(), 'pdae_set_deterministic', lib().pdae_set_deterministic(ws.data_ptr(), ws.numel()))

    def __exit__(self, *exc):
        torch.cuda.current_stream().synchronize()
        lib().pdae_ctx_set_current(self._prev)
        return False

    def close(self):
        _check(lib(), 'pdae_ctx_destroy', lib().pdae_ctx_destroy(self.handle))
        self._keep = []


_plan_cache = {}


def rows_gemm_plan(M, N, K, w_kn, may_split):
    """(cfg, splits, stream_blocks) of pdae_rows_gemm for a shape (host-side query, cached per arithmetic)."""
    key = (M, N, K, w_kn, may_split, lib().pdae_gemm_arith())
    hit = _plan_cache.get(key)
    if hit is None:
        handle = lib()
        cfg, splits, sb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _check(handle, 'pdae_rows_gemm_plan',
               handle.pdae_rows_gemm_plan(M, N, K, int(w_kn), int(may_split), ctypes.byref(cfg), ctypes.byref(splits),
                                          ctypes.byref(sb)))
        hit = _plan_cache[key] = (cfg.value, splits.value, sb.value)
    return hit


_wg_cache = {}

GEMM_F32MFMA, GEMM_BF16X3 = CONST['PDAE_GEMM_F32MFMA'], CONST['PDAE_GEMM_BF16X3']


def gemm_arith():
    """The row-GEMM family's arithmetic: GEMM_BF16X3 (exact-split bf16, default) or GEMM_F32MFMA (include/pdae.h)."""
    return lib().pdae_gemm_arith()


def set_gemm_arith(arith):
    """pdae_set_gemm_arith; the cached plans / workspace sizes answered for the old arithmetic are dropped."""
    handle = lib()
    _check(handle, 'pdae_set_gemm_arith', handle.pdae_set_gemm_arith(int(arith)))
    _plan_cache.clear()
    _wg_cache.clear()


def rows_wgrad_workspace(M, Ns, Ks):
    """workspace floats of pdae_rows_wgrad for a group of layers (cached)."""
    key = (M, tuple(Ns), tuple(Ks), lib().pdae_gemm_arith())
    hit = _wg_cache.get(key)
    if hit is None:
        handle = lib()
        floats = ctypes.c_longlong(0)
        _check(handle, 'pdae_rows_wgrad_workspace',
               handle.pdae_rows_wgrad_workspace(M, len(Ns), int_array(Ns), int_array(Ks), ctypes.byref(floats)))
        hit = _wg_cache[key] = floats.value
    return hit


def rows_wgrad(on, M, dYs, Xs, dWs, dbs, workspace):
    """pdae_rows_wgrad over lists of tensors (dbs entries may be None)."""
    call('pdae_rows_wgrad', on, M, len(dYs), ptr_array(dYs), ptr_array(Xs), ptr_array(dWs), ptr_array(dbs),
         int_array([t.shape[1] for t in dYs]), int_array([t.shape[1] for t in Xs]), ptr(workspace))


def edge_weights_multi(name, on, cos, cins, kps, srcs, dsts):
    """pdae_edge_weight_stack_multi / _unstack_multi over lists (HOST arrays of sizes and device pointers)."""
    call(name, on, len(cos), int_array(cos), int_array(cins), int_array(kps), ptr_array(srcs), ptr_array(dsts))


class AdamwSegment(ctypes.Structure):
    """pdae_adamw_segment of include/pdae.h."""
    _fields_ = [('offset', ctypes.c_longlong), ('count', ctypes.c_longlong), ('lr', ctypes.c_float),
                ('weight_decay', ctypes.c_float)]


ADAMW_MAX_SEGMENTS = CONST['PDAE_ADAMW_MAX_SEGMENTS']


def adamw_step_segments(flat_param, flat_grad, exp_avg, exp_avg_sq, segments, beta1, beta2, eps, step, gscale=None):
    """pdae_adamw_step_segments: segments = [(offset, count, lr, weight_decay)] over the flat buffers, 8 per launch
    (longer lists are cut); gscale: None or a one-element device tensor."""
    for t in (flat_grad, exp_avg, exp_avg_sq):
        if t.numel() != flat_param.numel():
            raise ValueError('adamw_step_segments: the four flat buffers must have one length')
        require(t, 'adamw_step_segments buffer', dim=1)
    require(flat_param, 'flat_param', dim=1)
    for i in range(0, len(segments), ADAMW_MAX_SEGMENTS):
        part = segments[i:i + ADAMW_MAX_SEGMENTS]
        table = (AdamwSegment * len(part))(*[AdamwSegment(int(o), int(c), float(lr), float(wd)) for o, c, lr, wd in part])
        call('pdae_adamw_step_segments', flat_param, flat_param.numel(), len(part), table, ptr(flat_param), ptr(flat_grad),
             ptr(exp_avg), ptr(exp_avg_sq), float(beta1), float(beta2), float(eps), int(step), ptr(gscale))


WGRAD_MULTI_MAX = 48


def multi_copy(pairs, strided=()):
    """pdae_multi_copy: pairs = [(dst, src)] contiguous fp32 device tensors of equal numel (src None: dst is zero-filled);
    strided = [(dst, src2d, cols)]: dst (contiguous, rows * cols elements) <- src2d[:, :cols] of a row-major 2-D tensor.
    One launch per 128 entries."""
    n = len(pairs) + len(strided)
    if n == 0:
        return
    on = pairs[0][0] if pairs else strided[0][0]
    for d, s_ in list(pairs) + [(d, s_) for d, s_, _ in strided]:
        for t in (d, s_):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != on.device):
                raise ValueError('multi_copy: contiguous fp32 tensors on one device')
    for d, s_ in pairs:
        if s_ is not None and d.numel() != s_.numel():
            raise ValueError('multi_copy: %r <- %r' % (tuple(d.shape), tuple(s_.shape)))
    for d, s_, c in strided:
        if s_.dim() != 2 or not 0 < c <= s_.shape[1] or d.numel() != s_.shape[0] * c:
            raise ValueError('multi_copy: %r <- %r[:, :%d]' % (tuple(d.shape), tuple(s_.shape), c))
    src = ptr_array([s_ for _, s_ in pairs] + [s_ for _, s_, _ in strided])
    dst = ptr_array([d for d, _ in pairs] + [d for d, _, _ in strided])
    cnt = (ctypes.c_longlong * n)(*([d.numel() for d, _ in pairs] + [d.numel() for d, _, _ in strided]))
    cols = sld = None
    if strided:
        cols = int_array([0] * len(pairs) + [c for _, _, c in strided])
        sld = int_array([0] * len(pairs) + [s_.shape[1] for _, s_, _ in strided])
    call('pdae_multi_copy', on, n, src, dst, cnt, cols, sld)


def rows_wgrad_multi(jobs):
    """pdae_rows_wgrad_multi: jobs = [(dY (M,N), X (M,K), dW (N,K), db (N,) or None)], every layer with its own row
    count, at most WGRAD_MULTI_MAX per launch (longer lists are cut).  The workspace is allocated here."""
    for i in range(0, len(jobs), WGRAD_MULTI_MAX):
        part = jobs[i:i + WGRAD_MULTI_MAX]
        n = len(part)
        Ms, Ns, Ks = (int_array(v) for v in ([j[0].shape[0] for j in part], [j[0].shape[1] for j in part],
                                             [j[1].shape[1] for j in part]))
        key = ('multi', tuple(Ms), tuple(Ns), tuple(Ks), lib().pdae_gemm_arith())
        floats = _wg_cache.get(key)
        if floats is None:
            f = ctypes.c_longlong(0)
            handle = lib()
            _check(handle, 'pdae_rows_wgrad_multi_workspace', handle.pdae_rows_wgrad_multi_workspace(n, Ms, Ns, Ks, ctypes.byref(f)))
            floats = _wg_cache[key] = f.value
        on = part[0][0]
        ws = torch.empty(max(floats, 1), device=on.device, dtype=torch.float32)
        call('pdae_rows_wgrad_multi', on, n, Ms, *(ptr_array([j[c] for j in part]) for c in range(4)), Ns, Ks, ptr(ws))
