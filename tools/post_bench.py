"""Posterior summaries at the north-star size: 65 536 chains x K = 500 kept draws x 10 rows (a
2.6 GB sample block), 6 rows selected (5 in log space, as ModelFramework.posterior_summary) and
all 15 pairs.

Times ``Engine.summarize`` on synthetic correlated log-normal rows built on the device: the whole
call, the marginal passes alone (no pairs) and so the pair passes by difference; the same
summaries written with torch on the same device (mean, var, amin, amax, histc, corrcoef of the
logged rows); the 32-chain x 1000-draw case; and the plan at 2, 4, 8 and 16 workgroups per CU and
row, each in a fresh process (OE_POST_WG_PER_CU is read once).  The one-read bound is the selected
rows' bytes over the HBM peak.  Prints one JSON line per measurement (``ms``: the call, host work
included; ``device_ms``: its launches, first to last, from the library's events); recorded in
DESIGN.md §3.14 and profiles/post/, not gated.

    python tools/post_bench.py [--chains 65536] [--kept 500] [--reps 5] [--no-torch] [--no-sweep]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0  # the HBM peak the project quotes
R_TOT, SEL, LOGS = 10, [0, 1, 2, 3, 4, 5], [1, 1, 1, 1, 1, 0]
QS, N_BINS, N_BINS2 = (0.025, 0.5, 0.975), 1024, 32


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


def draws(torch, dev, K, W, seed):
    """samples [K][R_TOT][W]: log-normal rows (sd 0.05 around exp(-18) .. exp(2)) sharing a
    component (so every pair is correlated), row 5 plain"""
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.empty((K, R_TOT, W), dtype=torch.float64, device=dev)
    level = torch.linspace(-18.0, 2.0, R_TOT, dtype=torch.float64, device=dev)[:, None]
    step = max(1, min(K, (1 << 24) // (R_TOT * W)))
    for k in range(0, K, step):
        n = min(step, K - k)
        z = torch.randn((n, R_TOT, W), generator=g, dtype=torch.float64, device=dev)
        x = 0.8 * z[:, :1, :] + 0.6 * z
        s[k:k + n] = torch.exp(level + 0.05 * x)
        s[k:k + n, 5] = x[:, 5]
    return s


def torch_summary(torch, s):
    """what torch offers for the same questions: moments, extremes, a histogram per row and the
    correlation matrix of the logged rows (no quantiles, no 2-D counts)"""
    x = s[:, SEL, :]
    x = torch.where(torch.tensor(LOGS, device=s.device, dtype=torch.bool)[None, :, None], x.log(), x)
    x = x.permute(1, 0, 2).reshape(len(SEL), -1)
    mean, var, lo, hi = x.mean(1), x.var(1, unbiased=True), x.amin(1), x.amax(1)
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    hist = [torch.histc(x[r], bins=N_BINS, min=float(lo_h[r]), max=float(hi_h[r])) for r in range(len(SEL))]
    corr = torch.corrcoef(x)
    return mean.cpu().numpy(), var.cpu().numpy(), torch.stack(hist).cpu().numpy(), corr.cpu().numpy()


def measure(a, emit):
    import torch
    from odelib_amd import _native as N
    from odelib_amd.engine import Engine, FitProblem

    eng = Engine(FitProblem(model_id=N.OE_MODEL_TWO_I, n_states=4, n_params=5, times=np.linspace(0.0, 1.0, 5)))
    wg = os.environ.get("OE_POST_WG_PER_CU", "2 (default)")
    shapes = [(a.kept, a.chains)] if a.one else [(a.kept, a.chains), (1000, 32)]
    for K, W in shapes:
        s = draws(torch, eng.dev, K, W, 1)
        sel_bytes = 8.0 * K * len(SEL) * W
        bound_ms = sel_bytes / (PEAK_TBS * 1e9)
        full = lambda: eng.summarize(s, rows=SEL, log_rows=LOGS, quantiles=QS, n_bins=N_BINS, pairs="all",  # noqa: E731
                                     n_bins2=N_BINS2, hist=True, hist2=True)
        marg = lambda: eng.summarize(s, rows=SEL, log_rows=LOGS, quantiles=QS, n_bins=N_BINS, pairs=None,  # noqa: E731
                                     hist=True)
        res = full()
        ms_m = timed(torch, marg, a.reps)
        dev_m = eng.last_kernel_ms()  # the last call's launches alone, first to last (library events)
        ms_f = timed(torch, full, a.reps)
        dev_f = eng.last_kernel_ms()
        emit(what="Engine.summarize, marginal passes (moments, histogram, quantiles)", wg_per_cu=wg, chains=W, kept=K,
             rows=R_TOT, selected=len(SEL), ms=round(ms_m, 4), device_ms=round(dev_m, 4), one_read_bound_ms=round(bound_ms, 4),
             passes_over_the_rows=2, bound_over_device_time=round(2 * bound_ms / dev_m, 4))
        emit(what="Engine.summarize, marginals and 15 pairs with 2-D counts", wg_per_cu=wg, chains=W, kept=K, ms=round(ms_f, 4),
             device_ms=round(dev_f, 4), pair_pass_device_ms=round(dev_f - dev_m, 4),
             pair_pass_reads_over_selected_rows=round(2 * len(res["pairs"]) / len(SEL), 2),
             pair_bound_over_device_time=round(2 * len(res["pairs"]) / len(SEL) * bound_ms / max(dev_f - dev_m, 1e-9), 4),
             corr_01=round(float(res["corr"][0]), 6), n=[int(v) for v in res["n"]])
        if not a.no_torch and not a.one:
            mean, var, hist, corr = torch_summary(torch, s)
            tms = timed(torch, lambda: torch_summary(torch, s), max(1, a.reps // 2))
            pc = np.array([corr[i, j] for i, j in res["pairs"]])
            emit(what="torch: mean, var, amin, amax, histc per row, corrcoef of the logged rows", chains=W, kept=K,
                 ms=round(tms, 4), torch_over_summarize=round(tms / ms_f, 2),
                 mean_max_abs_diff=float(np.max(np.abs(mean - res["mean"]))),
                 var_max_rel_diff=float(np.max(np.abs(var - res["m2"] / (res["n"] - 1)) / var)),
                 corr_max_abs_diff=float(np.max(np.abs(pc - res["corr"]))),
                 hist_counts_moved=int(np.abs(hist - res["hist"]).sum() // 2))
        del s
        torch.cuda.empty_cache()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--kept", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline")
    ap.add_argument("--no-sweep", action="store_true", help="skip the workgroups-per-CU sweep")
    ap.add_argument("--one", action="store_true", help="(the sweep's child) the large shape only, no baseline")
    a = ap.parse_args()

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    measure(a, emit)
    if a.one or a.no_sweep:
        return
    for wg in (2, 4, 8, 16):  # a fresh process each: the library reads the variable once
        env = dict(os.environ, OE_POST_WG_PER_CU=str(wg))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--chains", str(a.chains), "--kept", str(a.kept),
                        "--reps", str(a.reps)], env=env, check=True, timeout=600)


if __name__ == "__main__":
    main()
