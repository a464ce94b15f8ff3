"""ctypes binding of librhmc_post.so (include/rhmc_post.h): R-hat, effective
sample size and acceptance rates of recorded chains on the GPU, from device
pointers (the engine's MhRecord, torch tensors, padded rows) or host arrays.

Like capi, the library is required: importing this module without a built
librhmc_post.so raises (build: __graft_entry__.build() or
`make -C hmc-stellar-toy-model_amd/post`).  The package does not import this
module; rhmc_amd.diagnostics loads it on first use of a *_device function.
"""
import ctypes
import os

import numpy as np

from . import capi   # first: the HIP runtime is the one torch / the engine loaded

LIB_PATH = os.environ.get("RHMC_POST_LIB",
                          os.path.join(os.path.dirname(capi.LIB_PATH), "librhmc_post.so"))
ABI_VERSION = 1
OPT_TBLK = 1      # lags per pass (8, 16)
OPT_BLOCK = 2     # threads per workgroup (64, 128, 256)

EXPORTS = ("rhmc_post_abi_version", "rhmc_post_last_error", "rhmc_post_create",
           "rhmc_post_destroy", "rhmc_post_set_option", "rhmc_post_convergence_device",
           "rhmc_post_convergence", "rhmc_post_variogram_device", "rhmc_post_neff",
           "rhmc_post_acceptance_device", "rhmc_post_acceptance_fetch", "rhmc_post_acceptance")


class PostLayout(ctypes.Structure):
    """Mirror of `rhmc_post_layout`: strides in doubles, coordinate stride 1."""
    _fields_ = [(n, ctypes.c_int64) for n in ("n_iter", "n_chains", "D", "ld_iter", "ld_chain")]


class PostDetail(ctypes.Structure):
    """Mirror of `rhmc_post_detail`."""
    _fields_ = [("d_split_mean", ctypes.c_void_p), ("d_split_sd", ctypes.c_void_p),
                ("split_mean", ctypes.c_void_p), ("split_sd", ctypes.c_void_p),
                ("W", ctypes.c_void_p), ("B", ctypes.c_void_p), ("var", ctypes.c_void_p),
                ("lags_used", ctypes.c_void_p), ("passes", ctypes.c_int32),
                ("n", ctypes.c_int32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("librhmc_post.so not built at %s — run __graft_entry__.build()"
                          % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    P = ctypes.POINTER
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    sig = {
        "rhmc_post_abi_version": [],
        "rhmc_post_create": [ctypes.c_int, P(vp)],
        "rhmc_post_set_option": [vp, i32, i32],
        "rhmc_post_convergence_device": [vp, vp, P(PostLayout), i64, i64, i64, vp, vp,
                                         P(PostDetail), vp],
        "rhmc_post_convergence": [vp, vp, P(PostLayout), i64, i64, i64, vp, vp, P(PostDetail)],
        "rhmc_post_variogram_device": [vp, vp, P(PostLayout), i64, i64, i64, i64, vp, vp],
        "rhmc_post_neff": [i64, i64, ctypes.c_double, vp, i64, P(ctypes.c_double), P(i32)],
        "rhmc_post_acceptance_device": [vp, vp, i64, i64, i64, i64, i64, vp, vp],
        "rhmc_post_acceptance_fetch": [vp, vp, i64, i64, i64, i64, i64, vp, vp],
        "rhmc_post_acceptance": [vp, vp, i64, i64, i64, i64, i64, vp],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = args
    lib.rhmc_post_last_error.restype = ctypes.c_char_p
    lib.rhmc_post_last_error.argtypes = []
    lib.rhmc_post_destroy.restype = None
    lib.rhmc_post_destroy.argtypes = [vp]
    return lib


_lib = _load()


def lib():
    return _lib


def abi_version():
    return _lib.rhmc_post_abi_version()


def last_error():
    return _lib.rhmc_post_last_error().decode(errors="replace")


def _check(rc):
    if rc != 0:
        raise capi.RhmcError(rc, last_error())


def neff(m, n, var, V):
    """The lag search on given variograms V[i] = V_{i+1} -> (n_eff, decided)."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    out, dec = ctypes.c_double(0.), ctypes.c_int32(0)
    _check(_lib.rhmc_post_neff(int(m), int(n), float(var), V.ctypes.data if V.size else None,
                               V.size, ctypes.byref(out), ctypes.byref(dec)))
    return out.value, dec.value


def make_layout(n_iter, n_chains, D, ld_iter=None, ld_chain=None):
    """rhmc_post_layout; default strides: the engine's record [n_iter][n_chains][D]."""
    ld_chain = D if ld_chain is None else ld_chain
    ld_iter = n_chains * ld_chain if ld_iter is None else ld_iter
    return PostLayout(int(n_iter), int(n_chains), int(D), int(ld_iter), int(ld_chain))


class PostContext:
    """One GPU's post-processing context (rhmc_post_ctx): a grow-only device
    workspace.  Not for two threads at once."""

    def __init__(self, device=0, t_blk=None, block=None):
        h = ctypes.c_void_p()
        _check(_lib.rhmc_post_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = int(device)
        if t_blk is not None:
            self.set_option(OPT_TBLK, t_blk)
        if block is not None:
            self.set_option(OPT_BLOCK, block)

    def set_option(self, option, value):
        _check(_lib.rhmc_post_set_option(self._h, int(option), int(value)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.rhmc_post_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 - interpreter shutdown
            pass

    def _convergence(self, ptr, layout, warm_up, thin, max_lag, detail, stream, device):
        D, m = layout.D, 2 * layout.n_chains
        R, n_eff = np.empty(D), np.empty(D)
        det, out = None, None
        if detail:
            out = {"split_mean": np.empty((m, D)), "split_sd": np.empty((m, D)),
                   "W": np.empty(D), "B": np.empty(D), "var": np.empty(D),
                   "lags_used": np.empty(D, np.int32)}
            det = PostDetail(None, None, *[out[k].ctypes.data for k in
                                           ("split_mean", "split_sd", "W", "B", "var",
                                            "lags_used")], 0, 0)
        ref = None if det is None else ctypes.byref(det)
        if device:
            _check(_lib.rhmc_post_convergence_device(
                self._h, ctypes.c_void_p(ptr), ctypes.byref(layout), int(warm_up), int(thin),
                int(max_lag), R.ctypes.data, n_eff.ctypes.data, ref,
                ctypes.c_void_p(stream or 0)))
        else:
            _check(_lib.rhmc_post_convergence(
                self._h, ctypes.c_void_p(ptr), ctypes.byref(layout), int(warm_up), int(thin),
                int(max_lag), R.ctypes.data, n_eff.ctypes.data, ref))
        if detail:
            out.update(passes=det.passes, n=det.n, d_split_mean=det.d_split_mean,
                       d_split_sd=det.d_split_sd)
            return R, n_eff, out
        return R, n_eff

    def convergence_device(self, x_ptr, layout, warm_up=0, thin=1, max_lag=0, detail=False,
                           stream=None):
        """(R[D], n_eff[D]) of the fp64 device array at x_ptr (PostLayout);
        with detail a third item: dict of W, B, var, lags_used, split_mean,
        split_sd (host copies), d_split_mean / d_split_sd (device pointers,
        valid until the next call), passes, n.  Synchronises `stream`."""
        return self._convergence(x_ptr, layout, warm_up, thin, max_lag, detail, stream, True)

    def convergence(self, x, layout, warm_up=0, thin=1, max_lag=0, detail=False):
        """The same on a host float64 array holding the layout's extent."""
        x = np.asarray(x)
        if x.dtype != np.float64:
            raise TypeError("x must be float64, got %s" % x.dtype)
        return self._convergence(x.ctypes.data, layout, warm_up, thin, max_lag, detail, None,
                                 False)

    def variogram_device(self, x_ptr, layout, lag0, n_lags, warm_up=0, thin=1, stream=None):
        """V_t [n_lags][D] of the split sequences, t = lag0 .. lag0 + n_lags - 1."""
        V = np.empty((max(int(n_lags), 0), layout.D))
        _check(_lib.rhmc_post_variogram_device(
            self._h, ctypes.c_void_p(x_ptr), ctypes.byref(layout), int(warm_up), int(thin),
            int(lag0), int(n_lags), V.ctypes.data, ctypes.c_void_p(stream or 0)))
        return V

    def acceptance_device(self, accept_ptr, n_iter, n_chains, rate_ptr, ld_iter=None, start=-1,
                          end=-1, stream=None):
        """Rates of the int32 device record [n_iter][n_chains] into the device
        array rate_ptr [n_chains] (float64); asynchronous on `stream`."""
        _check(_lib.rhmc_post_acceptance_device(
            self._h, ctypes.c_void_p(accept_ptr), int(n_iter), int(n_chains),
            int(n_chains if ld_iter is None else ld_iter), int(start), int(end),
            ctypes.c_void_p(rate_ptr), ctypes.c_void_p(stream or 0)))

    def acceptance_fetch(self, accept_ptr, n_iter, n_chains, ld_iter=None, start=-1, end=-1,
                         stream=None):
        """Rates [n_chains] (NumPy) of the int32 device record; synchronises."""
        rate = np.empty(int(n_chains))
        _check(_lib.rhmc_post_acceptance_fetch(
            self._h, ctypes.c_void_p(accept_ptr), int(n_iter), int(n_chains),
            int(n_chains if ld_iter is None else ld_iter), int(start), int(end),
            rate.ctypes.data, ctypes.c_void_p(stream or 0)))
        return rate

    def acceptance(self, accept, start=-1, end=-1):
        """Rates [n_chains] of a host int32 record [n_iter][n_chains]."""
        a = np.ascontiguousarray(accept, dtype=np.int32)
        if a.ndim != 2:
            raise ValueError("accept must be [n_iter][n_chains]")
        rate = np.empty(a.shape[1])
        _check(_lib.rhmc_post_acceptance(self._h, a.ctypes.data, a.shape[0], a.shape[1],
                                         a.shape[1], int(start), int(end), rate.ctypes.data))
        return rate


_default = {}


def default_context(device=0):
    """A PostContext per device, created on first use and kept."""
    if device not in _default:
        _default[device] = PostContext(device)
    return _default[device]
