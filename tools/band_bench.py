"""Posterior band reductions on C1's shape (two_i, 65 536 rows, T = 1000: a 2.1 GB chunk).

Times, after >= 60 ms of warm-up launches, k_band_moments + k_band_merge and k_band_hist on a
trajectory written with and without non-temporal stores, the same reduction written with
torch (what a user without the kernels would write), and predict_band end to end.  Prints
one JSON line per measurement; recorded in DESIGN.md §3.9 and profiles/NOTES.md, not gated.

    python tools/band_bench.py [--rows 65536] [--big 1048576] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0  # the HBM peak the project quotes


def timed(torch, fn, reps):
    """ms per call of `reps` back-to-back calls, after >= 60 ms of the same launches"""
    t0 = time.perf_counter()
    n = 0
    while n < 3 or (time.perf_counter() - t0) < 0.06:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true", help="skip the torch baseline and predict_band")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import _demo_problem
    from odelib_amd import _native as N

    m, th = _demo_problem("rk4")
    eng = m.engine()
    T, S, W = len(m.times), 4, a.rows
    masks = m._band_masks()
    rs = np.random.RandomState(0)
    theta = (th[None, :] * np.exp(0.05 * rs.standard_normal((W, len(th))))).T.copy()
    y0 = np.repeat(np.asarray(m.get_inits(), float)[:, None], W, axis=1)
    nbytes = 8.0 * S * T * W
    acc = torch.empty((T, len(masks), 5), dtype=torch.float64, device=eng.dev)
    hist = torch.empty((T, len(masks), 1024), dtype=torch.int32, device=eng.dev)
    traj = eng.empty_traj(W)
    P = lambda t: t.data_ptr()  # noqa: E731

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    for nt in (True, False):
        eng.integrate(y0, theta, traj_out=traj, nt_stores=nt)
        eng.ctx.band_begin(masks, 1024, P(acc), P(hist))
        # once, right after the integrate that wrote the chunk (what Engine.band does) ...
        eng.ctx.band_moments(W, P(traj), P(acc))
        first_mom = eng.ctx.last_kernel_ms()
        eng.ctx.band_hist(W, P(traj), P(acc), P(hist))
        first_hist = eng.ctx.last_kernel_ms()
        # ... and back to back
        mom = timed(torch, lambda: eng.ctx.band_moments(W, P(traj), P(acc), N.OE_ASYNC), a.reps)
        hst = timed(torch, lambda: eng.ctx.band_hist(W, P(traj), P(acc), P(hist), N.OE_ASYNC), a.reps)
        for name, ms, first in (("k_band_moments+k_band_merge", mom, first_mom), ("k_band_hist", hst, first_hist)):
            emit(what=name, traj_nt_stores=nt, rows=W, T=T, ms=round(ms, 4), ms_first_after_integrate=round(first, 4),
                 read_TBs=round(nbytes / ms / 1e9, 3), of_peak=round(nbytes / ms / 1e9 / PEAK_TBS, 3))

    if a.kernels_only:
        return
    idx = [torch.tensor([s for s in range(S) if (int(k) >> s) & 1], device=eng.dev) for k in masks]

    def torch_reduce():
        out = []
        for ix in idx:
            l = traj[:, ix].sum(1).log()
            out.append((l.mean(1), l.var(1), l.amin(1), l.amax(1)))
        return out

    ms = timed(torch, torch_reduce, max(2, a.reps // 3))
    emit(what="torch: traj[:, idx].sum(1).log() -> mean, var, amin, amax (no histogram, no quantiles)", rows=W, T=T,
         ms=round(ms, 4), read_TBs=round(nbytes / ms / 1e9, 3))
    del traj, acc, hist
    torch.cuda.empty_cache()

    for rows in (a.rows, a.big):
        th_rows = th[None, :] * np.exp(0.05 * rs.standard_normal((rows, len(th))))
        m.predict_band(th_rows[:512])  # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        df = m.predict_band(th_rows)
        dt = time.perf_counter() - t0
        emit(what="predict_band end to end", rows=rows, T=T, seconds=round(dt, 4), n_min=int(df["n"].min()),
             n_status=int(df.attrs["n_status"]))


if __name__ == "__main__":
    main()
