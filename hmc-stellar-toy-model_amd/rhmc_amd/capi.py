"""ctypes binding of librhmc.so (include/rhmc.h).

Thin by design: argument marshalling, shape checks and error translation.
The library is REQUIRED — there is no CPU fallback; importing this module
without a built librhmc.so raises.  On a machine without a GPU the library
still loads (so its exports can be checked) but every compute entry point
returns an error.
"""
import ctypes
import os
import sys

import numpy as np

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RHMC_LIB", os.path.join(_PKG_DIR, "librhmc.so"))

RHMC_OK = 0
RHMC_ERR_ARG = -1
RHMC_ERR_HIP = -2
RHMC_ERR_NOMEM = -3
RHMC_ERR_UNSUPPORTED = -4

STATUS_NONFINITE = 1
STATUS_PLOOP_CAP = 2
STATUS_QLOOP_CAP = 4
STATUS_REFLECT_F = 8
STATUS_REFLECT_XY = 16
STATUS_NEAR_WALL = 32     # a reflection within 1e-12 of its wall
PEAK_CONVERGED = 256      # how a find_peaks seed stopped (RHMC_PEAK_*, include/rhmc.h)
PEAK_FAINT = 512
PEAK_CAP = 1024

OPT_KERNEL = 1            # rhmc_ctx_set_option (include/rhmc.h)
OPT_MH_FUSED = 2
OPT_WINDOW_SPLIT = 3        # waves per chain pair in leapfrog_kr (0: by batch size)
OPT_TABLES = 4              # where WinGG keeps its factor tables (diagnostic, rhmc.h)
OPT_PEAKS_FUSED = 5         # find_peaks: one-launch descent kernel where it exists
OPT_DT_LANES = 6            # dt_trials: lanes per task (0: the library's choice, 64, 256)
DT_GRAD_REFERENCE = 0       # rhmc_dt_opts.grad (RHMC_DT_GRAD_*, include/rhmc.h)
DT_GRAD_FULL = 1
TABLES_STREAM, TABLES_STREAM_POISON = 0, 1
CHAIN_UNIT = 0              # rhmc_chain_opts.metric (RHMC_CHAIN_*, include/rhmc.h)
CHAIN_DIAG = 1
# RHMC_KERNEL_* values by name
KERNELS = {"auto": 0, "generic": 1, "windowed": 2, "regwin": 3, "regwin32": 4,
           "regwin_f64": 5, "lane1": 6, "lane4": 7, "lane1_f64": 8, "pixmajor": 9,
           "multiwin": 10, "multiwin_notab": 11, "dense": 12}
# What a new Context selects unless told otherwise.  Production code leaves
# these alone; the parity tests set them (monkeypatch) to run the same inputs
# through every kernel family.  The library itself reads no environment.
DEFAULT_KERNEL = "auto"
DEFAULT_MH_FUSED = True

EXPORTS = ("rhmc_abi_version", "rhmc_device_count", "rhmc_last_error",
           "rhmc_ctx_create", "rhmc_ctx_set_image", "rhmc_ctx_image_device",
           "rhmc_ctx_destroy", "rhmc_ctx_synchronize", "rhmc_ctx_set_option",
           "rhmc_ctx_get_option", "rhmc_leapfrog",
           "rhmc_leapfrog_device", "rhmc_gradient", "rhmc_energy", "rhmc_energy_device",
           "rhmc_mh",
           "rhmc_mh_device", "rhmc_integrate", "rhmc_integrate_device",
           "rhmc_gen_image", "rhmc_gen_image_device", "rhmc_hmc_random",
           "rhmc_hmc_random_device", "rhmc_mh_scheduled", "rhmc_mh_scheduled_device",
           "rhmc_ragged_ok", "rhmc_leapfrog_ragged_device", "rhmc_energy_ragged_device",
           "rhmc_rows_copy_device", "rhmc_kinetic_rows_device",
           "rhmc_find_peaks", "rhmc_find_peaks_device",
           "rhmc_dt_trials", "rhmc_dt_trials_device",
           "rhmc_diag_random", "rhmc_diag_random_device",
           "rhmc_hess_derivs", "rhmc_hess_derivs_device",
           "rhmc_hess_random", "rhmc_hess_random_device",
           "rhmc_chain", "rhmc_chain_device")
ABI_VERSION = 4

V_FLUX_WALL = 1       # rhmc_energy f_pos bits (include/rhmc.h)
V_NO_POSCHECK = 2

SOLVER_IMPLICIT = 0
SOLVER_HMC = 1
SOLVER_RHMC_NAIVE = 2
SOLVER_RHMC_LEAPFROG = 3


class RhmcParams(ctypes.Structure):
    """Mirror of `rhmc_params` (include/rhmc.h)."""
    _fields_ = [
        ("dt", ctypes.c_double), ("delta", ctypes.c_double),
        ("B_count", ctypes.c_double), ("f_lim", ctypes.c_double),
        ("f_low", ctypes.c_double), ("fwhm_pix", ctypes.c_double),
        ("g_xx", ctypes.c_double), ("g_ff", ctypes.c_double),
        ("g_ff2", ctypes.c_double), ("g0", ctypes.c_double),
        ("g1", ctypes.c_double), ("g2", ctypes.c_double),
        ("alpha", ctypes.c_double), ("beta", ctypes.c_double),
        ("Vc_r_pow", ctypes.c_double), ("V_prior_const", ctypes.c_double),
        ("counter_max", ctypes.c_int32), ("use_prior", ctypes.c_int32),
        ("use_Vc", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class MhRecord(ctypes.Structure):
    """Mirror of `rhmc_mh_record` (include/rhmc.h); all fields nullable."""
    _fields_ = [("q_chain", ctypes.c_void_p), ("E_chain", ctypes.c_void_p),
                ("V_chain", ctypes.c_void_p), ("T_chain", ctypes.c_void_p),
                ("accept", ctypes.c_void_p)]


class MhSchedule(ctypes.Structure):
    """Mirror of `rhmc_mh_schedule` (include/rhmc.h): host arrays."""
    _fields_ = [("g_ff2", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("n_g_ff2", ctypes.c_int32), ("n_beta", ctypes.c_int32)]


class PeaksOpts(ctypes.Structure):
    """Mirror of `rhmc_peaks_opts` (include/rhmc.h)."""
    _fields_ = [("f_lim", ctypes.c_double), ("dt_f_coeff", ctypes.c_double),
                ("dt_xy_coeff", ctypes.c_double), ("rel_tol", ctypes.c_double),
                ("n_step", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def make_peaks_opts(f_lim, n_step=1000, dt_f_coeff=1e-1, dt_xy_coeff=1e-1, rel_tol=1e-9):
    """find_peaks' arguments (samplers.py:129-130; rel_tol is its hard-wired 1e-9)."""
    return PeaksOpts(float(f_lim), float(dt_f_coeff), float(dt_xy_coeff), float(rel_tol),
                     int(n_step), 0)


class DtOpts(ctypes.Structure):
    """Mirror of `rhmc_dt_opts` (include/rhmc.h)."""
    _fields_ = [("n_iter", ctypes.c_int32), ("grad", ctypes.c_int32),
                ("steps_min", ctypes.c_int32), ("steps_max", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 2)]


class DtRecord(ctypes.Structure):
    """Mirror of `rhmc_dt_record` (include/rhmc.h)."""
    _fields_ = [("dE", ctypes.c_void_p), ("accept", ctypes.c_void_p), ("q", ctypes.c_void_p),
                ("z", ctypes.c_void_p), ("steps", ctypes.c_void_p), ("lnu", ctypes.c_void_p)]


def make_dt_opts(n_iter=10, grad=DT_GRAD_REFERENCE, steps_min=10, steps_max=50):
    """HMC_find_best_dt's Niter_per_trial, the gradient form ("reference" /
    "full" or a DT_GRAD_* value) and the range of the device's step draws."""
    if isinstance(grad, str):
        grad = {"reference": DT_GRAD_REFERENCE, "full": DT_GRAD_FULL}[grad]
    return DtOpts(int(n_iter), int(grad), int(steps_min), int(steps_max), (0, 0))


class DiagOpts(ctypes.Structure):
    """Mirror of `rhmc_diag_opts` (include/rhmc.h)."""
    _fields_ = [("dt", ctypes.c_double), ("factor1", ctypes.c_double),
                ("trace_rows", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class HessOpts(ctypes.Structure):
    """Mirror of `rhmc_hess_opts` (include/rhmc.h)."""
    _fields_ = [("dt_f", ctypes.c_double), ("dt_xy", ctypes.c_double),
                ("reserved", ctypes.c_int32 * 2)]


class ChainOpts(ctypes.Structure):
    """Mirror of `rhmc_chain_opts` (include/rhmc.h)."""
    _fields_ = [("dt_global", ctypes.c_double), ("factor1", ctypes.c_double),
                ("metric", ctypes.c_int32), ("n_iter", ctypes.c_int32),
                ("iter0", ctypes.c_int32), ("steps_min", ctypes.c_int32),
                ("steps_max", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ChainRecord(ctypes.Structure):
    """Mirror of `rhmc_chain_record` (include/rhmc.h); all fields nullable."""
    _fields_ = [("q_chain", ctypes.c_void_p), ("E_chain", ctypes.c_void_p),
                ("dE_chain", ctypes.c_void_p), ("accept", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("z", ctypes.c_void_p),
                ("steps", ctypes.c_void_p), ("lnu", ctypes.c_void_p)]


def make_chain_opts(metric, n_iter, dt_global=0., factor1=0., iter0=0, steps_min=10,
                    steps_max=50):
    """rhmc_chain's options: metric "unit" / "diag" or a CHAIN_* value, Niter,
    RHMC_random_diag's one step and factor1, the number of the iteration before
    the call's first and the range of the device's length draws."""
    if isinstance(metric, str):
        metric = {"unit": CHAIN_UNIT, "diag": CHAIN_DIAG}[metric]
    return ChainOpts(float(dt_global), float(factor1), int(metric), int(n_iter), int(iter0),
                     int(steps_min), int(steps_max), 0)


def make_schedule(schedule_g_ff2=None, schedule_beta=None):
    """(MhSchedule, arrays to keep alive) for run_RHMC's schedule_g_ff2 /
    schedule_beta (sampler_RHMC.py:1010-1016), or (None, ()) without one."""
    if schedule_g_ff2 is None and schedule_beta is None:
        return None, ()
    g = None if schedule_g_ff2 is None else _f64(np.ravel(schedule_g_ff2), "schedule_g_ff2")
    b = None if schedule_beta is None else _f64(np.ravel(schedule_beta), "schedule_beta")
    sc = MhSchedule(None if g is None or g.size == 0 else g.ctypes.data,
                    None if b is None or b.size == 0 else b.ctypes.data,
                    0 if g is None else g.size, 0 if b is None else b.size)
    return sc, (g, b)


class RhmcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("librhmc error %d: %s" % (code, msg))
        self.code = code


def _load():
    if "torch" in sys.modules or os.environ.get("RHMC_IMPORT_TORCH") == "1":
        # Bind to the HIP runtime torch already loaded (same soname), so device
        # pointers and streams from torch are valid here.
        import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError("librhmc.so not built at %s — run __graft_entry__.build()" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    P = ctypes.POINTER
    c_dp = P(ctypes.c_double)
    c_ip = P(ctypes.c_int32)
    vp = ctypes.c_void_p
    sig = {
        "rhmc_abi_version": (ctypes.c_int, []),
        "rhmc_device_count": (ctypes.c_int, [P(ctypes.c_int)]),
        "rhmc_last_error": (ctypes.c_char_p, []),
        "rhmc_ctx_create": (ctypes.c_int, [ctypes.c_int, c_dp, ctypes.c_int32, ctypes.c_int32, P(vp)]),
        "rhmc_ctx_set_image": (ctypes.c_int, [vp, c_dp, ctypes.c_int32, ctypes.c_int32]),
        "rhmc_ctx_image_device": (ctypes.c_int, [vp, P(vp)]),
        "rhmc_ctx_destroy": (None, [vp]),
        "rhmc_ctx_synchronize": (ctypes.c_int, [vp]),
        "rhmc_ctx_set_option": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.c_int32]),
        "rhmc_ctx_get_option": (ctypes.c_int, [vp, ctypes.c_int32, P(ctypes.c_int32)]),
        "rhmc_leapfrog": (ctypes.c_int, [vp, P(RhmcParams), c_dp, c_dp, ctypes.c_int64,
                                         ctypes.c_int32, ctypes.c_int32, c_ip, c_ip]),
        "rhmc_leapfrog_device": (ctypes.c_int, [vp, P(RhmcParams), vp, vp, ctypes.c_int64,
                                                ctypes.c_int32, ctypes.c_int32, vp, vp, vp]),
        "rhmc_gradient": (ctypes.c_int, [vp, P(RhmcParams), c_dp, c_dp, ctypes.c_int64,
                                         ctypes.c_int32, ctypes.c_int32]),
        "rhmc_energy": (ctypes.c_int, [vp, P(RhmcParams), c_dp, c_dp, c_dp, c_dp,
                                       ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
        "rhmc_energy_device": (ctypes.c_int, [vp, P(RhmcParams), vp, vp, vp, vp, ctypes.c_int64,
                                              ctypes.c_int32, ctypes.c_int32, vp]),
        "rhmc_integrate": (ctypes.c_int, [vp, P(RhmcParams), ctypes.c_int32, c_dp, c_dp,
                                          ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_int32, c_ip]),
        "rhmc_integrate_device": (ctypes.c_int, [vp, P(RhmcParams), ctypes.c_int32, vp, vp,
                                                 ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.c_int32, vp, vp]),
        "rhmc_mh": (ctypes.c_int, [vp, P(RhmcParams), c_dp, ctypes.c_int64, ctypes.c_int32,
                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_dp, c_dp,
                                   ctypes.c_uint64, P(MhRecord)]),
        "rhmc_mh_device": (ctypes.c_int, [vp, P(RhmcParams), vp, ctypes.c_int64, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp,
                                          ctypes.c_uint64, P(MhRecord), vp]),
        "rhmc_mh_scheduled": (ctypes.c_int, [vp, P(RhmcParams), c_dp, ctypes.c_int64,
                                             ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_int32, c_dp, c_dp, ctypes.c_uint64,
                                             P(MhRecord), P(MhSchedule)]),
        "rhmc_mh_scheduled_device": (ctypes.c_int, [vp, P(RhmcParams), vp, ctypes.c_int64,
                                                    ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.c_int32, ctypes.c_int32, vp, vp,
                                                    ctypes.c_uint64, P(MhRecord), P(MhSchedule),
                                                    vp]),
        "rhmc_hmc_random": (ctypes.c_int, [vp, P(RhmcParams), c_dp, c_dp, c_dp, c_ip,
                                           ctypes.c_int64, ctypes.c_int32, c_ip]),
        "rhmc_hmc_random_device": (ctypes.c_int, [vp, P(RhmcParams), vp, vp, vp, vp,
                                                  ctypes.c_int64, ctypes.c_int32, vp, vp]),
        "rhmc_gen_image": (ctypes.c_int, [vp, P(RhmcParams), c_dp, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, c_dp,
                                          ctypes.c_int32]),
        "rhmc_gen_image_device": (ctypes.c_int, [vp, P(RhmcParams), vp, ctypes.c_int32,
                                                 ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.c_uint64, vp, vp]),
        "rhmc_ragged_ok": (ctypes.c_int, [vp, P(RhmcParams), ctypes.c_int32, P(ctypes.c_int32)]),
        "rhmc_leapfrog_ragged_device": (ctypes.c_int, [vp, P(RhmcParams), vp, vp, ctypes.c_int64,
                                                       vp, vp, ctypes.c_int64, ctypes.c_int32,
                                                       ctypes.c_int32, ctypes.c_int32, vp]),
        "rhmc_energy_ragged_device": (ctypes.c_int, [vp, P(RhmcParams), vp, ctypes.c_int64, vp,
                                                     vp, ctypes.c_int64, ctypes.c_int32,
                                                     ctypes.c_int32, ctypes.c_int32, vp, vp]),
        "rhmc_rows_copy_device": (ctypes.c_int, [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64,
                                                 vp, ctypes.c_int64, ctypes.c_int32, vp]),
        "rhmc_kinetic_rows_device": (ctypes.c_int, [vp, P(RhmcParams), vp, vp, ctypes.c_int64,
                                                    vp, vp, vp, ctypes.c_int64, vp, vp]),
        "rhmc_find_peaks": (ctypes.c_int, [vp, P(RhmcParams), P(PeaksOpts), c_dp, ctypes.c_int64,
                                           c_ip, c_ip, c_dp]),
        "rhmc_find_peaks_device": (ctypes.c_int, [vp, P(RhmcParams), P(PeaksOpts), vp,
                                                  ctypes.c_int64, vp, vp, vp, vp]),
        "rhmc_dt_trials": (ctypes.c_int, [vp, P(RhmcParams), P(DtOpts), vp, ctypes.c_int32, vp, vp,
                                          vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_uint64, vp,
                                          vp, P(DtRecord)]),
        "rhmc_dt_trials_device": (ctypes.c_int, [vp, P(RhmcParams), P(DtOpts), vp, ctypes.c_int32,
                                                 vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp,
                                                 ctypes.c_uint64, vp, vp, P(DtRecord), vp]),
        "rhmc_diag_random": (ctypes.c_int, [vp, P(RhmcParams), P(DiagOpts), vp, vp, vp,
                                            ctypes.c_int64, ctypes.c_int32, vp, vp]),
        "rhmc_diag_random_device": (ctypes.c_int, [vp, P(RhmcParams), P(DiagOpts), vp, vp, vp,
                                                   ctypes.c_int64, ctypes.c_int32, vp, vp, vp]),
        "rhmc_hess_derivs": (ctypes.c_int, [vp, P(RhmcParams), vp, vp, vp, vp, vp,
                                            ctypes.c_int64, ctypes.c_int32]),
        "rhmc_hess_derivs_device": (ctypes.c_int, [vp, P(RhmcParams), vp, vp, vp, vp, vp,
                                                   ctypes.c_int64, ctypes.c_int32, vp]),
        "rhmc_hess_random": (ctypes.c_int, [vp, P(RhmcParams), P(HessOpts), vp, vp, vp,
                                            ctypes.c_int64, ctypes.c_int32, vp, vp, vp, vp, vp]),
        "rhmc_hess_random_device": (ctypes.c_int, [vp, P(RhmcParams), P(HessOpts), vp, vp, vp,
                                                   ctypes.c_int64, ctypes.c_int32, vp, vp, vp, vp,
                                                   vp, vp]),
        "rhmc_chain": (ctypes.c_int, [vp, P(RhmcParams), P(ChainOpts), vp, vp, ctypes.c_int64,
                                      ctypes.c_int32, vp, vp, vp, ctypes.c_uint64, vp,
                                      P(ChainRecord)]),
        "rhmc_chain_device": (ctypes.c_int, [vp, P(RhmcParams), P(ChainOpts), vp, vp,
                                             ctypes.c_int64, ctypes.c_int32, vp, vp, vp,
                                             ctypes.c_uint64, vp, P(ChainRecord), vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = _load()


def lib():
    return _lib


def abi_version():
    return _lib.rhmc_abi_version()


def device_count():
    n = ctypes.c_int(0)
    _lib.rhmc_device_count(ctypes.byref(n))
    return n.value


def device_available():
    return device_count() > 0


def _check(rc):
    if rc != RHMC_OK:
        raise RhmcError(rc, _lib.rhmc_last_error().decode(errors="replace"))


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _iptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _f64(a, name):
    a = np.asarray(a)
    if a.dtype != np.float64:
        raise TypeError("%s must be float64, got %s" % (name, a.dtype))
    return np.ascontiguousarray(a)


def make_params(dt, delta, counter_max, B_count, f_lim, f_low, fwhm_pix, g_xx, g_ff,
                g_ff2, g0, g1, g2, use_prior=False, alpha=2., use_Vc=False, beta=1.,
                Vc_r_pow=1., V_prior_const=0.):
    return RhmcParams(float(dt), float(delta), float(B_count), float(f_lim), float(f_low),
                      float(fwhm_pix), float(g_xx), float(g_ff), float(g_ff2), float(g0),
                      float(g1), float(g2), float(alpha), float(beta), float(Vc_r_pow),
                      float(V_prior_const), int(counter_max), int(bool(use_prior)),
                      int(bool(use_Vc)), 0)


class Context:
    """One GPU + one data image (rhmc_ctx)."""

    def __init__(self, D, device=0, kernel=None, mh_fused=None):
        """D: the data image, or None for a context whose image comes from
        gen_image(..., install=True).  kernel: a KERNELS name (default
        DEFAULT_KERNEL), mh_fused: one-launch MH where available (default
        DEFAULT_MH_FUSED)."""
        h = ctypes.c_void_p()
        if D is None:
            _check(_lib.rhmc_ctx_create(int(device), None, 0, 0, ctypes.byref(h)))
            self.shape = None
        else:
            D = _f64(D, "D")
            if D.ndim != 2:
                raise ValueError("D must be 2-D")
            _check(_lib.rhmc_ctx_create(int(device), _dptr(D), D.shape[0], D.shape[1],
                                        ctypes.byref(h)))
            self.shape = D.shape
        self._h = h
        self.device = device
        self.set_kernel(DEFAULT_KERNEL if kernel is None else kernel)
        self.set_option(OPT_MH_FUSED, int(bool(DEFAULT_MH_FUSED if mh_fused is None
                                               else mh_fused)))

    def set_option(self, option, value):
        _check(_lib.rhmc_ctx_set_option(self._h, int(option), int(value)))

    def get_option(self, option):
        v = ctypes.c_int32()
        _check(_lib.rhmc_ctx_get_option(self._h, int(option), ctypes.byref(v)))
        return v.value

    def set_kernel(self, name):
        """Kernel family for this context's compute calls (KERNELS name)."""
        if name not in KERNELS:
            raise ValueError("unknown kernel %r (one of %s)" % (name, ", ".join(KERNELS)))
        self.set_option(OPT_KERNEL, KERNELS[name])

    @property
    def handle(self):
        return self._h

    def set_image(self, D):
        D = _f64(D, "D")
        _check(_lib.rhmc_ctx_set_image(self._h, _dptr(D), D.shape[0], D.shape[1]))
        self.shape = D.shape

    def image_device_ptr(self):
        p = ctypes.c_void_p()
        _check(_lib.rhmc_ctx_image_device(self._h, ctypes.byref(p)))
        return p.value

    def synchronize(self):
        _check(_lib.rhmc_ctx_synchronize(self._h))

    def close(self):
        if getattr(self, "_h", None):
            _lib.rhmc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- compute ----------------------------------------------------------
    def leapfrog(self, params, q, p, n_steps, K=None, return_info=False):
        """n_steps fused RHMC_single_step()s; q, p: [n_chains, 3K] (or [3K]).
        Returns new (q, p) arrays (inputs are not mutated, like the reference)."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        p2 = np.array(p, dtype=np.float64, order="C", copy=True)
        if q2.shape != p2.shape:
            raise ValueError("q and p shapes differ")
        single = q2.ndim == 1
        q2 = q2.reshape(-1, q2.shape[-1]) if not single else q2.reshape(1, -1)
        p2 = p2.reshape(q2.shape)
        if q2.shape[1] % 3:
            raise ValueError("last dimension must be 3K")
        K = q2.shape[1] // 3 if K is None else K
        n = q2.shape[0]
        it = np.zeros((n, 2), np.int32)
        st = np.zeros(n, np.int32)
        _check(_lib.rhmc_leapfrog(self._h, ctypes.byref(params), _dptr(q2), _dptr(p2), n,
                                  int(K), int(n_steps), _iptr(it), _iptr(st)))
        if single:
            q2, p2, it, st = q2[0], p2[0], it[0], st[0]
        if return_info:
            return q2, p2, it, st
        return q2, p2

    def leapfrog_device(self, params, q_ptr, p_ptr, n_chains, K, n_steps, iters_ptr=None,
                        status_ptr=None, stream=None):
        _check(_lib.rhmc_leapfrog_device(self._h, ctypes.byref(params), ctypes.c_void_p(q_ptr),
                                         ctypes.c_void_p(p_ptr), int(n_chains), int(K),
                                         int(n_steps), ctypes.c_void_p(iters_ptr or 0),
                                         ctypes.c_void_p(status_ptr or 0),
                                         ctypes.c_void_p(stream or 0)))

    def energy_device(self, params, q_ptr, p_ptr, V_ptr, T_ptr, n_chains, K, f_pos=0,
                      stream=None):
        """rhmc_energy_device: device pointers (p_ptr / T_ptr may be 0), f_pos bits."""
        _check(_lib.rhmc_energy_device(self._h, ctypes.byref(params), ctypes.c_void_p(q_ptr),
                                       ctypes.c_void_p(p_ptr or 0), ctypes.c_void_p(V_ptr or 0),
                                       ctypes.c_void_p(T_ptr or 0), int(n_chains), int(K),
                                       int(f_pos), ctypes.c_void_p(stream or 0)))

    # ---- ragged chain sets (ABI 4; device pointers, asynchronous on `stream`)
    def ragged_ok(self, params, K):
        """Whether chains of K stars can share ragged launches on this image."""
        ok = ctypes.c_int32(0)
        _check(_lib.rhmc_ragged_ok(self._h, ctypes.byref(params), int(K), ctypes.byref(ok)))
        return bool(ok.value)

    def leapfrog_ragged_device(self, params, q_ptr, p_ptr, ld, rows_ptr, K_ptr, n, K_min, K_max,
                               n_steps, stream=None):
        _check(_lib.rhmc_leapfrog_ragged_device(
            self._h, ctypes.byref(params), ctypes.c_void_p(q_ptr), ctypes.c_void_p(p_ptr),
            int(ld), ctypes.c_void_p(rows_ptr or 0), ctypes.c_void_p(K_ptr), int(n), int(K_min),
            int(K_max), int(n_steps), ctypes.c_void_p(stream or 0)))

    def energy_ragged_device(self, params, q_ptr, ld, rows_ptr, K_ptr, n, K_min, K_max, f_pos,
                             V_ptr, stream=None):
        _check(_lib.rhmc_energy_ragged_device(
            self._h, ctypes.byref(params), ctypes.c_void_p(q_ptr), int(ld),
            ctypes.c_void_p(rows_ptr or 0), ctypes.c_void_p(K_ptr), int(n), int(K_min),
            int(K_max), int(f_pos), ctypes.c_void_p(V_ptr), ctypes.c_void_p(stream or 0)))

    def rows_copy_device(self, src_ptr, ld_src, src_rows_ptr, dst_ptr, ld_dst, dst_rows_ptr, n,
                         width, stream=None):
        _check(_lib.rhmc_rows_copy_device(
            self._h, ctypes.c_void_p(src_ptr), int(ld_src), ctypes.c_void_p(src_rows_ptr or 0),
            ctypes.c_void_p(dst_ptr), int(ld_dst), ctypes.c_void_p(dst_rows_ptr or 0), int(n),
            int(width), ctypes.c_void_p(stream or 0)))

    def kinetic_rows_device(self, params, q_ptr, p_ptr, ld, K_ptr, z_ptr, zoff_ptr, n, T_ptr,
                            stream=None):
        _check(_lib.rhmc_kinetic_rows_device(
            self._h, ctypes.byref(params), ctypes.c_void_p(q_ptr), ctypes.c_void_p(p_ptr),
            int(ld), ctypes.c_void_p(K_ptr), ctypes.c_void_p(z_ptr or 0),
            ctypes.c_void_p(zoff_ptr or 0), int(n), ctypes.c_void_p(T_ptr),
            ctypes.c_void_p(stream or 0)))

    def gradient(self, params, q, kind=0):
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        g = np.empty_like(q2)
        _check(_lib.rhmc_gradient(self._h, ctypes.byref(params), _dptr(q2), _dptr(g),
                                  q2.shape[0], q2.shape[1] // 3, int(kind)))
        return g[0] if single else g

    def energy(self, params, q, p=None, f_pos=False, pos_check=True):
        """Returns (V, T); T is None when p is None.  pos_check=False drops the
        position support check (samplers.lightsource_gym.V has none)."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        n = q2.shape[0]
        V = np.empty(n)
        T = None
        pp = None
        if p is not None:
            pp = np.array(p, dtype=np.float64, order="C", copy=True).reshape(q2.shape)
            T = np.empty(n)
        _check(_lib.rhmc_energy(self._h, ctypes.byref(params), _dptr(q2),
                                None if pp is None else _dptr(pp), _dptr(V),
                                None if T is None else _dptr(T), n, q2.shape[1] // 3,
                                (V_FLUX_WALL if f_pos else 0) | (0 if pos_check else V_NO_POSCHECK)))
        if single:
            return V[0], (None if T is None else T[0])
        return V, T

    def mh(self, params, q, n_iter, n_steps, f_pos=True, z=None, u=None, seed=0, record=True,
           schedule_g_ff2=None, schedule_beta=None):
        """n_iter MH iterations (run_RHMC move-0 branch) of n_steps leapfrog steps
        on every chain of q [n_chains, 3K].  z [n_iter, n_chains, 3K] / u
        [n_iter, n_chains]: host randoms (None = Philox on device).
        schedule_g_ff2 / schedule_beta: run_RHMC's per-iteration schedules
        (rhmc_mh_scheduled).  Returns a dict with the final q and, when record,
        q_chain/E_chain/V_chain/T_chain [n_iter, n_chains(, 3K)] and accept
        [n_iter, n_chains]."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        n, d = q2.shape
        zz = None if z is None else _f64(z, "z").reshape(n_iter, n, d)
        uu = None if u is None else _f64(u, "u").reshape(n_iter, n)
        out = {}
        rec = None
        if record:
            out["q_chain"] = np.empty((n_iter, n, d))
            for k in ("E_chain", "V_chain", "T_chain"):
                out[k] = np.empty((n_iter, n))
            out["accept"] = np.empty((n_iter, n), np.int32)
            rec = MhRecord(out["q_chain"].ctypes.data, out["E_chain"].ctypes.data,
                           out["V_chain"].ctypes.data, out["T_chain"].ctypes.data,
                           out["accept"].ctypes.data)
        sc, keep = make_schedule(schedule_g_ff2, schedule_beta)
        _check(_lib.rhmc_mh_scheduled(
            self._h, ctypes.byref(params), _dptr(q2), n, d // 3, int(n_iter), int(n_steps),
            int(bool(f_pos)), None if zz is None else _dptr(zz),
            None if uu is None else _dptr(uu), ctypes.c_uint64(int(seed)),
            None if rec is None else ctypes.byref(rec), None if sc is None else ctypes.byref(sc)))
        del keep
        out["q"] = q2[0] if single else q2
        return out

    def mh_device(self, params, q_ptr, n_chains, K, n_iter, n_steps, f_pos=True, z_ptr=None,
                  u_ptr=None, seed=0, record=None, stream=None, schedule_g_ff2=None,
                  schedule_beta=None):
        """Device-pointer variant (asynchronous on `stream`); record: MhRecord of
        device pointers or None; schedules: host arrays (read during the call)."""
        sc, keep = make_schedule(schedule_g_ff2, schedule_beta)
        _check(_lib.rhmc_mh_scheduled_device(
            self._h, ctypes.byref(params), ctypes.c_void_p(q_ptr), int(n_chains), int(K),
            int(n_iter), int(n_steps), int(bool(f_pos)), ctypes.c_void_p(z_ptr or 0),
            ctypes.c_void_p(u_ptr or 0), ctypes.c_uint64(int(seed)),
            None if record is None else ctypes.byref(record),
            None if sc is None else ctypes.byref(sc), ctypes.c_void_p(stream or 0)))
        del keep

    def integrate(self, params, solver, q, p, n_steps, f_pos=False, return_status=False):
        """n_steps steps of integrator `solver` (SOLVER_*); returns new (q, p)."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        p2 = np.array(p, dtype=np.float64, order="C", copy=True)
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        p2 = p2.reshape(q2.shape)
        st = np.zeros(q2.shape[0], np.int32)
        _check(_lib.rhmc_integrate(self._h, ctypes.byref(params), int(solver), _dptr(q2),
                                   _dptr(p2), q2.shape[0], q2.shape[1] // 3, int(n_steps),
                                   int(bool(f_pos)), _iptr(st)))
        if single:
            q2, p2, st = q2[0], p2[0], st[0]
        return (q2, p2, st) if return_status else (q2, p2)

    def hmc_random_device(self, params, dt_ptr, q_ptr, p_ptr, steps_ptr, n_chains, K,
                          status_ptr=None, stream=None):
        """Device-pointer rhmc_hmc_random (asynchronous on `stream`)."""
        _check(_lib.rhmc_hmc_random_device(self._h, ctypes.byref(params),
                                           ctypes.c_void_p(dt_ptr), ctypes.c_void_p(q_ptr),
                                           ctypes.c_void_p(p_ptr), ctypes.c_void_p(steps_ptr),
                                           int(n_chains), int(K),
                                           ctypes.c_void_p(status_ptr or 0),
                                           ctypes.c_void_p(stream or 0)))

    def integrate_device(self, params, solver, q_ptr, p_ptr, n_chains, K, n_steps, f_pos=False,
                         status_ptr=None, stream=None):
        """Device-pointer rhmc_integrate (asynchronous on `stream`)."""
        _check(_lib.rhmc_integrate_device(self._h, ctypes.byref(params), int(solver),
                                          ctypes.c_void_p(q_ptr), ctypes.c_void_p(p_ptr),
                                          int(n_chains), int(K), int(n_steps),
                                          int(bool(f_pos)), ctypes.c_void_p(status_ptr or 0),
                                          ctypes.c_void_p(stream or 0)))

    def hmc_random(self, params, dt, q, p, steps, return_status=False):
        """samplers.HMC_random trajectories (rhmc_hmc_random): per-coordinate
        step vector dt [3K], steps[c] >= 1 leapfrog steps for chain c, flux
        wall at params.f_lim.  Returns new (q, p) (p is the input momentum on
        chains whose last step flipped — the reference's stale-p quirk)."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        p2 = np.array(p, dtype=np.float64, order="C", copy=True)
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        p2 = p2.reshape(q2.shape)
        K = q2.shape[1] // 3
        dt2 = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, np.float64), (3 * K,)))
        st = np.zeros(q2.shape[0], np.int32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(steps, np.int32), (q2.shape[0],)))
        _check(_lib.rhmc_hmc_random(self._h, ctypes.byref(params), _dptr(dt2), _dptr(q2),
                                    _dptr(p2), _iptr(n), q2.shape[0], K, _iptr(st)))
        if single:
            q2, p2, st = q2[0], p2[0], st[0]
        return (q2, p2, st) if return_status else (q2, p2)

    def diag_random(self, params, dt, factor1, q, p, steps, return_status=False, trace=False):
        """samplers.RHMC_random_diag trajectories (rhmc_diag_random): leapfrog
        under the mass matrix diag(1/f, f factor1, f factor1) per star with the
        one step dt, steps[c] >= 1 steps for chain c, flux wall at
        params.f_lim.  Returns new (q, p) (p is the input momentum on chains
        whose last step flipped — the reference's stale-p quirk), then the
        status words with return_status, then with trace=True q after every
        step [n_chains, max(steps) + 1, 3K] (row 0 the start, NaN past a
        chain's own trajectory; a 1-D q gives [steps + 1, 3K])."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        p2 = np.array(p, dtype=np.float64, order="C", copy=True)
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        p2 = p2.reshape(q2.shape)
        K = q2.shape[1] // 3
        st = np.zeros(q2.shape[0], np.int32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(steps, np.int32), (q2.shape[0],)))
        tr, rows = None, 0
        if trace:
            rows = int(n.max()) + 1 if n.size else 1
            tr = np.full((q2.shape[0], rows, 3 * K), np.nan)
        opts = DiagOpts(float(dt), float(factor1), rows, 0)
        vp = ctypes.c_void_p
        _check(_lib.rhmc_diag_random(self._h, ctypes.byref(params), ctypes.byref(opts),
                                     vp(q2.ctypes.data), vp(p2.ctypes.data), vp(n.ctypes.data),
                                     q2.shape[0], K, vp(st.ctypes.data),
                                     None if tr is None else vp(tr.ctypes.data)))
        if single:
            q2, p2, st = q2[0], p2[0], st[0]
            tr = None if tr is None else tr[0]
        out = (q2, p2) + ((st,) if return_status else ()) + ((tr,) if trace else ())
        return out

    def diag_random_device(self, params, dt, factor1, q_ptr, p_ptr, steps_ptr, n_chains, K,
                           status_ptr=None, trace_ptr=None, trace_rows=0, stream=None):
        """Device-pointer rhmc_diag_random (asynchronous on `stream`)."""
        opts = DiagOpts(float(dt), float(factor1), int(trace_rows), 0)
        vp = ctypes.c_void_p
        _check(_lib.rhmc_diag_random_device(self._h, ctypes.byref(params), ctypes.byref(opts),
                                            vp(q_ptr), vp(p_ptr), vp(steps_ptr), int(n_chains),
                                            int(K), vp(status_ptr or 0), vp(trace_ptr or 0),
                                            vp(stream or 0)))

    def hess_derivs(self, params, q, V=False):
        """RHMC_efficient_computation's derivative sets (rhmc_hess_derivs) at q
        [n_chains, 3K] or [3K]: (dVdq, dVdqq, dVdqqq), each shaped like q, with
        V=True also V = -sum(D ln Lambda - Lambda) per chain.  No wall check."""
        q2 = _f64(q, "q")
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        n, K = q2.shape[0], q2.shape[1] // 3
        d1, d2, d3 = np.empty_like(q2), np.empty_like(q2), np.empty_like(q2)
        Vv = np.empty(n) if V else None
        vp = ctypes.c_void_p
        _check(_lib.rhmc_hess_derivs(self._h, ctypes.byref(params), vp(q2.ctypes.data),
                                     vp(d1.ctypes.data), vp(d2.ctypes.data), vp(d3.ctypes.data),
                                     None if Vv is None else vp(Vv.ctypes.data), n, K))
        if single:
            d1, d2, d3 = d1[0], d2[0], d3[0]
            Vv = None if Vv is None else Vv[0]
        return (d1, d2, d3, Vv) if V else (d1, d2, d3)

    def hess_derivs_device(self, params, q_ptr, n_chains, K, dVdq_ptr=None, dVdqq_ptr=None,
                           dVdqqq_ptr=None, V_ptr=None, stream=None):
        """Device-pointer rhmc_hess_derivs (asynchronous on `stream`)."""
        vp = ctypes.c_void_p
        _check(_lib.rhmc_hess_derivs_device(self._h, ctypes.byref(params), vp(q_ptr),
                                            vp(dVdq_ptr or 0), vp(dVdqq_ptr or 0),
                                            vp(dVdqqq_ptr or 0), vp(V_ptr or 0), int(n_chains),
                                            int(K), vp(stream or 0)))

    def hess_random(self, params, dt_f, dt_xy, q, p, steps, derivs=False):
        """samplers.RHMC_random trajectories (rhmc_hess_random): leapfrog under
        the metric diag(dVdqq) with the steps (dt_f, dt_xy, dt_xy) per star,
        steps[c] >= 1 steps for chain c, the flux wall at params.f_lim >= 0.
        Returns (q, p, status, steps_done): the end state, p_half as the
        reference leaves it, the RHMC_STATUS_* words and the completed steps
        (below steps[c] iff the trajectory broke off); with derivs=True also
        (dVdq, dVdqq, dVdqqq) at the end state."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        p2 = np.array(p, dtype=np.float64, order="C", copy=True)
        single = q2.ndim == 1
        q2 = q2.reshape(1, -1) if single else q2.reshape(-1, q2.shape[-1])
        p2 = p2.reshape(q2.shape)
        n_ch, K = q2.shape[0], q2.shape[1] // 3
        st = np.zeros(n_ch, np.int32)
        done = np.zeros(n_ch, np.int32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(steps, np.int32), (n_ch,)))
        d = [np.empty_like(q2) for _ in range(3)] if derivs else [None] * 3
        opts = HessOpts(float(dt_f), float(dt_xy), (ctypes.c_int32 * 2)(0, 0))
        vp = ctypes.c_void_p
        _check(_lib.rhmc_hess_random(self._h, ctypes.byref(params), ctypes.byref(opts),
                                     vp(q2.ctypes.data), vp(p2.ctypes.data), vp(n.ctypes.data),
                                     n_ch, K, vp(st.ctypes.data), vp(done.ctypes.data),
                                     *[None if a is None else vp(a.ctypes.data) for a in d]))
        if single:
            q2, p2, st, done = q2[0], p2[0], st[0], done[0]
            d = [None if a is None else a[0] for a in d]
        return (q2, p2, st, done) + (tuple(d) if derivs else ())

    def hess_random_device(self, params, dt_f, dt_xy, q_ptr, p_ptr, steps_ptr, n_chains, K,
                           status_ptr=None, steps_done_ptr=None, dVdq_ptr=None, dVdqq_ptr=None,
                           dVdqqq_ptr=None, stream=None):
        """Device-pointer rhmc_hess_random (asynchronous on `stream`)."""
        opts = HessOpts(float(dt_f), float(dt_xy), (ctypes.c_int32 * 2)(0, 0))
        vp = ctypes.c_void_p
        _check(_lib.rhmc_hess_random_device(self._h, ctypes.byref(params), ctypes.byref(opts),
                                            vp(q_ptr), vp(p_ptr), vp(steps_ptr), int(n_chains),
                                            int(K), vp(status_ptr or 0), vp(steps_done_ptr or 0),
                                            vp(dVdq_ptr or 0), vp(dVdqq_ptr or 0),
                                            vp(dVdqqq_ptr or 0), vp(stream or 0)))

    def chain(self, params, opts, q, dt=None, z=None, steps=None, lnu=None, seed=0,
              stream_id=None, record=True):
        """The whole MH chain of samplers.HMC_random / RHMC_random_diag
        (rhmc_chain) on the chains q [n, 3K]; opts: make_chain_opts(...); dt
        [3K]: HMC_random's step vector (unit metric).  Draws: z [n_iter + 1, n,
        3K], steps [n_iter, n] and lnu [n_iter, n] (all three), or none for the
        device's Philox draws under `seed` and stream_id [n] (None: the chain
        index).  Returns a dict with the final q and, when record, q_chain,
        z [n_iter + 1, n, 3K], E_chain, dE_chain [n_iter + 1, n] and accept,
        status, steps, lnu [n_iter, n]; record may also name the members
        wanted (the others are neither written nor copied back)."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True)
        q2 = q2.reshape(1, -1) if q2.ndim == 1 else q2.reshape(-1, q2.shape[-1])
        n, d = q2.shape
        ni = opts.n_iter
        keep = []

        def arr(a, dtype, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype).reshape(shape)
            keep.append(a)
            return a

        def ptr(a):
            return None if a is None else ctypes.c_void_p(a.ctypes.data)

        dt = None if dt is None else arr(np.broadcast_to(np.asarray(dt, np.float64), (d,)),
                                         np.float64, (d,))
        z = arr(z, np.float64, (ni + 1, n, d))
        steps = arr(steps, np.int32, (ni, n))
        lnu = arr(lnu, np.float64, (ni, n))
        stream_id = arr(stream_id, np.uint64, (n,))
        out, rec = {}, None
        if record:
            shapes = dict(q_chain=((ni + 1, n, d), np.float64), E_chain=((ni + 1, n), np.float64),
                          dE_chain=((ni + 1, n), np.float64), accept=((ni, n), np.int32),
                          status=((ni, n), np.int32), z=((ni + 1, n, d), np.float64),
                          steps=((ni, n), np.int32), lnu=((ni, n), np.float64))
            names = list(shapes) if record is True else list(record)
            out = {k: np.zeros(*shapes[k]) for k in names}
            rec = ChainRecord(*[out[k].ctypes.data if k in out else None for k in shapes])
        _check(_lib.rhmc_chain(self._h, ctypes.byref(params), ctypes.byref(opts), ptr(dt),
                               ptr(q2), n, d // 3, ptr(z), ptr(steps), ptr(lnu),
                               ctypes.c_uint64(int(seed)), ptr(stream_id),
                               None if rec is None else ctypes.byref(rec)))
        del keep
        out["q"] = q2
        return out

    def chain_device(self, params, opts, q_ptr, n, K, dt_ptr=None, z_ptr=None, steps_ptr=None,
                     lnu_ptr=None, seed=0, stream_id_ptr=None, record=None, stream=None):
        """Device-pointer rhmc_chain (asynchronous on `stream`); record: a
        ChainRecord of device pointers or None."""
        vp = ctypes.c_void_p
        _check(_lib.rhmc_chain_device(
            self._h, ctypes.byref(params), ctypes.byref(opts), vp(dt_ptr or 0), vp(q_ptr), int(n),
            int(K), vp(z_ptr or 0), vp(steps_ptr or 0), vp(lnu_ptr or 0),
            ctypes.c_uint64(int(seed)), vp(stream_id_ptr or 0),
            None if record is None else ctypes.byref(record), vp(stream or 0)))

    def find_peaks(self, params, opts, q):
        """find_peaks' seed descent (rhmc_find_peaks) on seeds q [n, 3] =
        (f counts, x, y); opts: make_peaks_opts(...).  Returns (q, steps,
        status, V): the final states, the gradient evaluations, PEAK_* (|
        STATUS_NONFINITE) and the last V evaluated per seed."""
        q2 = np.array(q, dtype=np.float64, order="C", copy=True).reshape(-1, 3)
        n = q2.shape[0]
        steps = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        V = np.zeros(n)
        _check(_lib.rhmc_find_peaks(self._h, ctypes.byref(params), ctypes.byref(opts), _dptr(q2),
                                    n, _iptr(steps), _iptr(status), _dptr(V)))
        return q2, steps, status, V

    def find_peaks_device(self, params, opts, q_ptr, n, steps_ptr=None, status_ptr=None,
                          V_ptr=None, stream=None):
        """Device-pointer rhmc_find_peaks (asynchronous on `stream`)."""
        _check(_lib.rhmc_find_peaks_device(self._h, ctypes.byref(params), ctypes.byref(opts),
                                           ctypes.c_void_p(q_ptr), int(n),
                                           ctypes.c_void_p(steps_ptr or 0),
                                           ctypes.c_void_p(status_ptr or 0),
                                           ctypes.c_void_p(V_ptr or 0),
                                           ctypes.c_void_p(stream or 0)))

    def dt_trials(self, params, opts, bg, bg_index, q0, dt, flux_only=None, z=None, steps=None,
                  lnu=None, seed=0, stream_id=None, record=False):
        """The trials of HMC_find_best_dt's search (rhmc_dt_trials): task t
        starts at q0[t] with the steps dt[t] against the background image
        bg[bg_index[t]]; opts: make_dt_opts(...).  Draws: z [n, n_iter, 3],
        steps [n, n_iter] and lnu [n, n_iter] (all three), or none and
        stream_id [n] for the device's Philox draws under `seed`.  Returns
        n_accept [n], with record=True (n_accept, dict of dE, accept, q, z,
        steps, lnu per iteration)."""
        bg = np.ascontiguousarray(bg, np.float64)
        if bg.ndim == 2:
            bg = bg[None]
        if bg.ndim != 3 or bg.shape[1:] != tuple(self.shape):
            raise ValueError("bg must be [n_bg, %d, %d]" % tuple(self.shape))
        q0 = np.ascontiguousarray(q0, np.float64).reshape(-1, 3)
        n = q0.shape[0]
        ni = opts.n_iter
        dt = np.ascontiguousarray(dt, np.float64).reshape(n, 3)
        bg_index = np.ascontiguousarray(bg_index, np.int32).reshape(n)
        keep = [bg, q0, dt, bg_index]

        def arr(a, dtype, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype).reshape(shape)
            keep.append(a)
            return a

        def ptr(a):
            return None if a is None else ctypes.c_void_p(a.ctypes.data)

        flux_only = arr(flux_only, np.int32, (n,))
        z = arr(z, np.float64, (n, ni, 3))
        steps = arr(steps, np.int32, (n, ni))
        lnu = arr(lnu, np.float64, (n, ni))
        stream_id = arr(stream_id, np.uint64, (n,))
        n_accept = np.zeros(n, np.int32)
        rec, out = None, None
        if record:
            out = dict(dE=np.zeros((n, ni)), accept=np.zeros((n, ni), np.int32),
                       q=np.zeros((n, ni, 3)), z=np.zeros((n, ni, 3)),
                       steps=np.zeros((n, ni), np.int32), lnu=np.zeros((n, ni)))
            rec = DtRecord(*[out[k].ctypes.data for k in ("dE", "accept", "q", "z", "steps", "lnu")])
        _check(_lib.rhmc_dt_trials(
            self._h, ctypes.byref(params), ctypes.byref(opts), ptr(bg), bg.shape[0], ptr(bg_index),
            ptr(q0), ptr(dt), ptr(flux_only), n, ptr(z), ptr(steps), ptr(lnu),
            ctypes.c_uint64(int(seed)), ptr(stream_id), ptr(n_accept),
            None if rec is None else ctypes.byref(rec)))
        del keep
        return (n_accept, out) if record else n_accept

    def dt_trials_device(self, params, opts, bg_ptr, n_bg, bg_index_ptr, q0_ptr, dt_ptr, n,
                         flux_only_ptr=None, z_ptr=None, steps_ptr=None, lnu_ptr=None, seed=0,
                         stream_id_ptr=None, n_accept_ptr=None, record=None, stream=None):
        """Device-pointer rhmc_dt_trials (asynchronous on `stream`); record: a
        DtRecord of device pointers or None."""
        vp = ctypes.c_void_p
        _check(_lib.rhmc_dt_trials_device(
            self._h, ctypes.byref(params), ctypes.byref(opts), vp(bg_ptr), int(n_bg),
            vp(bg_index_ptr), vp(q0_ptr), vp(dt_ptr), vp(flux_only_ptr or 0), int(n),
            vp(z_ptr or 0), vp(steps_ptr or 0), vp(lnu_ptr or 0), ctypes.c_uint64(int(seed)),
            vp(stream_id_ptr or 0), vp(n_accept_ptr or 0),
            None if record is None else ctypes.byref(record), vp(stream or 0)))

    def gen_image(self, params, q, rows, cols, n_real=0, seed=0, install=False):
        """Model image (n_real=0, gen_model) or n_real Poisson realisations of it
        (gen_mock_data / gen_noise_profile) for stars q [K, 3] (flux in counts,
        x, y).  Returns [rows, cols] or [n_real, rows, cols]; install=True also
        makes image 0 this context's data image."""
        qq = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1, 3))
        K = qq.shape[0]
        out = np.empty((n_real, rows, cols) if n_real > 0 else (rows, cols))
        _check(_lib.rhmc_gen_image(self._h, ctypes.byref(params), _dptr(qq) if K else None,
                                   K, int(rows), int(cols), int(n_real),
                                   ctypes.c_uint64(int(seed)), _dptr(out), int(bool(install))))
        if install:
            self.shape = (rows, cols)
        return out

    def gen_image_device(self, params, q_ptr, K, rows, cols, n_real, seed, out_ptr, stream=None):
        _check(_lib.rhmc_gen_image_device(self._h, ctypes.byref(params),
                                          ctypes.c_void_p(q_ptr or 0), int(K), int(rows),
                                          int(cols), int(n_real), ctypes.c_uint64(int(seed)),
                                          ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)))
