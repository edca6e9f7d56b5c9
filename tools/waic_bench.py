"""Posterior-wide model comparison on C1's shape (two_i, 65 536 rows, T = 1000, the notebook's
observations).

Times, after >= 60 ms of warm-up launches and back to back: k_waic_accum + k_waic_merge alone on
a trajectory chunk already on the device (with and without storing the terms), the whole
Engine.waic (integrate, accumulate, finish, the copy of the results), the integrate alone, and
the same reduction written with torch on the same device: gather the observed rows, log,
torch.logsumexp, var.  Prints one JSON line per measurement; recorded in DESIGN.md §3.11 and
profiles/waic/, not gated.

    python tools/waic_bench.py [--rows 65536] [--reps 10]
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
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import _demo_problem
    from odelib_amd import _native as N

    m, th = _demo_problem("rk4")
    eng = m.engine()
    fp = eng.problem
    T, S, W, n_obs = len(m.times), fp.n_states, a.rows, fp.n_obs
    rs = np.random.RandomState(0)
    theta = torch.as_tensor((th[None, :] * np.exp(0.05 * rs.standard_normal((W, len(th))))).T.copy(), device=eng.dev)
    y0 = torch.as_tensor(np.repeat(np.asarray(m.get_inits(), float)[:, None], W, axis=1), device=eng.dev)
    acc = torch.empty((n_obs, 5), dtype=torch.float64, device=eng.dev)
    point = torch.empty((n_obs, 6), dtype=torch.float64, device=eng.dev)
    summary = torch.empty(8, dtype=torch.float64, device=eng.dev)
    terms = torch.empty((n_obs, W), dtype=torch.float64, device=eng.dev)
    traj = eng.empty_traj(W)
    P = lambda t: t.data_ptr()  # noqa: E731
    # what the pass must read: each observation's states of its grid row; and the whole chunk
    read_bytes = 8.0 * W * sum(bin(int(k)).count("1") for k in fp.obs_mask)
    chunk_bytes = 8.0 * S * T * W

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    eng.integrate(y0, theta, traj_out=traj)
    eng.ctx.waic_begin(P(acc))
    for name, tp in (("k_waic_accum+k_waic_merge", None), ("k_waic_accum+k_waic_merge, terms stored", P(terms))):
        ms = timed(torch, lambda: eng.ctx.waic_accum(W, P(traj), P(acc), tp, W, 0, N.OE_ASYNC), a.reps)
        emit(what=name, rows=W, T=T, n_obs=n_obs, ms=round(ms, 4), read_GB=round(read_bytes / 1e9, 4),
             read_TBs=round(read_bytes / ms / 1e9, 3), of_peak=round(read_bytes / ms / 1e9 / PEAK_TBS, 3))
    ms = timed(torch, lambda: eng.ctx.waic_finish(P(acc), P(point), P(summary), N.OE_ASYNC), a.reps)
    emit(what="k_waic_finish", n_obs=n_obs, ms=round(ms, 4))

    ms_int = timed(torch, lambda: eng.integrate(y0, theta, traj_out=traj, sync=False, timing=False), a.reps)
    emit(what="integrate alone (the chunk written)", rows=W, T=T, ms=round(ms_int, 4), chunk_GB=round(chunk_bytes / 1e9, 3),
         write_TBs=round(chunk_bytes / ms_int / 1e9, 3))
    del traj, terms
    torch.cuda.empty_cache()
    res = {}

    def whole():
        res["r"] = eng.waic(y0, theta)

    ms_all = timed(torch, whole, max(2, a.reps // 2))
    r = res["r"]
    emit(what="Engine.waic (integrate + accumulate + finish + results to the host)", rows=W, T=T, n_obs=n_obs,
         ms=round(ms_all, 4), integrate_share=round(ms_int / ms_all, 3), elpd_waic=r["summary"]["elpd_waic"],
         p_waic=r["summary"]["p_waic"], se_elpd=r["summary"]["se_elpd"], n_rows_min=r["summary"]["n_rows_min"])

    # torch on the same device, from the same chunk: gather the observed rows, log, logsumexp, var
    traj = eng.empty_traj(W)
    eng.integrate(y0, theta, traj_out=traj)
    tidx = torch.as_tensor(fp.obs_tidx.astype(np.int64), device=eng.dev)
    groups = {}
    for k, mask in enumerate(fp.obs_mask):
        groups.setdefault(int(mask), []).append(k)
    O = torch.as_tensor(fp.obs_log, device=eng.dev)
    two_s2 = torch.as_tensor(2.0 * fp.obs_logsigma ** 2, device=eng.dev)
    c_o = torch.as_tensor(-(np.log(fp.obs_logsigma) + 0.5 * np.log(2.0 * np.pi)), device=eng.dev)

    def torch_waic():
        lppd = torch.empty(n_obs, dtype=torch.float64, device=eng.dev)
        p = torch.empty(n_obs, dtype=torch.float64, device=eng.dev)
        for mask, ks in groups.items():
            ks_t = torch.as_tensor(ks, device=eng.dev)
            states = torch.as_tensor([s for s in range(S) if (mask >> s) & 1], device=eng.dev)
            c = traj[tidx[ks_t]][:, states].sum(1)          # [obs of the mask][W]
            d = O[ks_t, None] - c.log()
            e = -(d * d) / two_s2[ks_t, None]
            lppd[ks_t] = torch.logsumexp(e, 1) - float(np.log(W)) + c_o[ks_t]
            p[ks_t] = e.var(1)
        return lppd, p

    ms_t = timed(torch, torch_waic, a.reps)
    lppd_t, p_t = torch_waic()
    torch.cuda.synchronize()
    emit(what="torch: gather the observed rows, log, logsumexp, var (no validity mask, no terms)", rows=W, T=T,
         n_obs=n_obs, ms=round(ms_t, 4),
         lppd_max_abs_diff=float(np.abs(lppd_t.cpu().numpy() - r["lppd"]).max()),
         p_waic_max_rel_diff=float((np.abs(p_t.cpu().numpy() - r["p_waic"]) / np.maximum(r["p_waic"], 1e-300)).max()))


if __name__ == "__main__":
    main()
