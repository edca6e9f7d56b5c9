"""MCMC convergence diagnostics at the north-star size: 65 536 chains x K = 500 kept draws x 10
rows (a 2.6 GB sample block), 6 rows selected (5 in log space, as ModelFramework.convergence).

Times ``Engine.diagnose`` on synthetic AR(1) chains built on the device (phi = 0.5: the walk
stops in the first lag block; phi = 0.95: slow chains, every lag block runs), the same
estimator written with torch on the same device (FFT autocovariance), and the 32-chain case.
The one-read bound is the selected rows' bytes over the HBM peak.  Prints one JSON line per
measurement (``ms``: the call, host work included; ``device_ms``: its kernels, first launch to
last, from the library's events); recorded in DESIGN.md §3.10 and profiles/diag/, not gated.

    python tools/diag_bench.py [--chains 65536] [--kept 500] [--reps 5]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0  # the HBM peak the project quotes
R_TOT, SEL, LOGS = 10, [0, 1, 2, 3, 4, 5], [1, 1, 1, 1, 1, 0]


def timed(torch, fn, reps):
    """ms per call of `reps` back-to-back calls, after >= 60 ms of the same launches"""
    t0 = time.perf_counter()
    n = 0
    while n < 2 or (time.perf_counter() - t0) < 0.06:
        fn()
        torch.cuda.synchronize()
        n += 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def chains(torch, dev, K, W, phi, seed):
    """samples [K][R_TOT][W]: log-normal AR(1) rows (sd 0.05 around exp(-18) .. exp(2)), row 5 plain"""
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.empty((K, R_TOT, W), dtype=torch.float64, device=dev)
    x = torch.randn((R_TOT, W), generator=g, dtype=torch.float64, device=dev)
    level = torch.linspace(-18.0, 2.0, R_TOT, dtype=torch.float64, device=dev)[:, None]
    c = math.sqrt(1.0 - phi * phi)
    for k in range(K):
        if k:
            x = phi * x + c * torch.randn((R_TOT, W), generator=g, dtype=torch.float64, device=dev)
        s[k] = torch.exp(level + 0.05 * x)
        s[k, 5] = x[5]
    return s


def torch_diagnose(torch, s, max_lag):
    """the estimator of oe_diag_run in torch: FFT autocovariance of every split chain, the
    sums across chains, rho; Geyer's walk on the host from the [n_sel][max_lag + 1] result"""
    K = s.shape[0]
    n = K // 2
    x = s[:, SEL, :]
    x = torch.where(torch.tensor(LOGS, device=s.device, dtype=torch.bool)[None, :, None], x.log(), x)
    h = torch.stack((x[:n], x[K - n:]), 0)                      # [2][n][sel][W]
    m = h.mean(1, keepdim=True)
    c = h - m
    f = torch.fft.rfft(c, n=2 * n, dim=1)
    acov = torch.fft.irfft(f * f.conj(), n=2 * n, dim=1)[:, :max_lag + 1] / n   # [2][L+1][sel][W]
    M = 2 * s.shape[2]
    abar = acov.sum((0, 3)) / M                                 # [L+1][sel]
    Wbar = abar[0] * n / (n - 1)
    B = n * m.squeeze(1).var((0, 2), unbiased=True)
    varp = (n - 1) / n * Wbar + B / n
    rho = (1.0 - (Wbar[None] - abar) / varp[None]).T.cpu().numpy()
    rho[:, 0] = 1.0
    tau = []
    for r in rho:
        k, prev, tot = 0, math.inf, 0.0
        while 2 * k + 1 <= max_lag and r[2 * k] + r[2 * k + 1] >= 0:
            prev = min(prev, r[2 * k] + r[2 * k + 1])
            tot += prev
            k += 1
        tau.append(max(-1.0 + 2.0 * tot, 1.0 / math.log10(M * n)))
    return torch.sqrt(varp / Wbar).cpu().numpy(), np.asarray(tau)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--kept", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline")
    a = ap.parse_args()
    import torch
    from odelib_amd import _native as N
    from odelib_amd.engine import Engine, FitProblem

    eng = Engine(FitProblem(model_id=N.OE_MODEL_TWO_I, n_states=4, n_params=5, times=np.linspace(0.0, 1.0, 5)))
    K = a.kept
    max_lag = K // 2 - 1

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    for W, phi in ((a.chains, 0.5), (a.chains, 0.95), (32, 0.95)):
        s = chains(torch, eng.dev, K, W, phi, 1)
        sel_bytes = 8.0 * K * len(SEL) * W
        bound_ms = sel_bytes / (PEAK_TBS * 1e9)
        res = eng.diagnose(s, rows=SEL, log_rows=LOGS)
        ms = timed(torch, lambda: eng.diagnose(s, rows=SEL, log_rows=LOGS), a.reps)
        dev_ms = eng.last_kernel_ms()  # the last call's launches alone, first to last (library events)
        emit(what="Engine.diagnose", chains=W, kept=K, rows=R_TOT, selected=len(SEL), phi=phi, ms=round(ms, 4),
             device_ms=round(dev_ms, 4), bound_over_device_time=round(bound_ms / dev_ms, 4),
             one_read_bound_ms=round(bound_ms, 4), bound_over_time=round(bound_ms / ms, 4),
             stop_lag=res["stop_lag"].tolist(), truncated=res["truncated"].tolist(),
             rhat=[round(float(v), 4) for v in res["rhat"]], tau=[round(float(v), 3) for v in res["tau"]])
        if not a.no_torch:
            rhat, tau = torch_diagnose(torch, s, max_lag)
            tms = timed(torch, lambda: torch_diagnose(torch, s, max_lag), max(1, a.reps // 2))
            emit(what="torch: rfft autocovariance of every split chain, sums across chains, host walk", chains=W, kept=K,
                 phi=phi, ms=round(tms, 4), torch_over_diagnose=round(tms / ms, 2),
                 rhat_max_abs_diff=float(np.max(np.abs(rhat - res["rhat"]))),
                 tau_max_rel_diff=float(np.max(np.abs(tau - res["tau"]) / res["tau"])))
        del s
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
