#!/usr/bin/env python3
"""Per-phase cycle split of the register-window kernel (tools only).

Needs the phase-timing library: `make -C hmc-stellar-toy-model_amd prof`
(-DRHMC_PHASE_PROF -> build/variants/lib_prof.so), whose register-window
launches write cycles per step per wave over the chain state: the gradient,
kicks + reflection + p-loop, q-loop, flux metric + closing update, and inside
the gradient the window check, PSF factors, pixel loop and moments +
reductions (fenced s_memtime reads).
usage: RHMC_LIB=build/variants/lib_prof.so python tools/phase_prof.py [n_chains]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hmc-stellar-toy-model_amd"))
import numpy as np  # noqa: E402

from rhmc_amd import capi, workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
kern = "profr"
STEPS = 200
wl = workloads.make("C2", n_chains=n)
P = capi.make_params(**wl.params)
ctx = capi.Context(wl.D)
# Through the host-buffer entry point, which returns when the launch is done:
# every launch starts from wl.q0, wl.p0.  (Until this change the two launches
# went through device pointers on a side stream; the second one's momentum
# buffer was the first one's freed state buffer, which the first launch, still
# running, then overwrote with its cycle counts.  The chains of the reported
# launch therefore flew across the image: every gradient reloaded its window
# and the far chains took the direct PSF factors.)
for _ in range(2):
    qq, pp, itn, stw = ctx.leapfrog(P, wl.q0, wl.p0, STEPS, return_info=True)
itn = itn.astype(float)
if kern.startswith("profr"):
    ph = [qq[:, 0].mean(), qq[:, 1].mean(), qq[:, 2].mean(), pp[:, 0].mean()]
    print("%s n=%d cycles/step: gradient %.0f  kicks+p-loop %.0f  q-loop %.0f  flux+tail %.0f"
          "  total %.0f" % (kern, n, ph[0], ph[1], ph[2], ph[3], sum(ph)))
    g4 = [itn[:, 1].mean(), pp[:, 1].mean(), pp[:, 2].mean(), itn[:, 0].mean()]
    print("  gradient split: window check %.0f  PSF factors %.0f  pixel loop %.0f  "
          "moments + reductions %.0f" % tuple(g4))
    # status: gradients whose wave reloaded its window | their mean check cycles << 16
    sw = stw.astype(np.int64) & 0xFFFFFFFF
    nre, cre = (sw & 0xFFFF).astype(float), (sw >> 16).astype(float)
    grads = STEPS + 1.0                            # gradients per launch
    rest = (itn[:, 1] * STEPS - nre * cre) / (grads - nre)
    print("  window check: %.1f %% of gradients reload, %.0f cycles each; the others %.0f"
          % (100.0 * nre.mean() / grads, cre[nre > 0].mean(), rest.mean()))
else:
    print("%s n=%d cycles/step: gradient %.0f  rest %.0f  total %.0f" % (
        kern, n, itn[:, 0].mean(), itn[:, 1].mean(), itn.sum(1).mean()))
