"""PSIS-LOO on the two_i data (the notebook's observations, T = 1000) at 10^6 posterior rows.

Times, after >= 60 ms of warm-up calls and back to back: the whole Engine.waic with the terms
stored (integrate in chunks, accumulate, finish, results to the host) and oe_loo_run alone on
those terms where they lie (six select passes, the gather, the fit, the summary), with the HBM
bytes the stage must read: terms once per select pass and once for the gather.  Prints one JSON
line per measurement; recorded in DESIGN.md §3.13 and profiles/loo/, not gated.

    python tools/loo_bench.py [--rows 1000000] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.waic_bench import PEAK_TBS, timed  # noqa: E402

SELECT_PASSES = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import _demo_problem
    from odelib_amd import _native as N

    m, th = _demo_problem("rk4")
    eng = m.engine()
    fp = eng.problem
    T, W, n_obs = len(m.times), a.rows, fp.n_obs
    rs = np.random.RandomState(0)
    theta = torch.as_tensor((th[None, :] * np.exp(0.05 * rs.standard_normal((W, len(th))))).T.copy(), device=eng.dev)
    y0 = torch.as_tensor(np.repeat(np.asarray(m.get_inits(), float)[:, None], W, axis=1), device=eng.dev)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    res = {}

    def waic_terms():
        res["w"] = eng.waic(y0, theta, terms=True)

    ms_waic = timed(torch, waic_terms, max(2, a.reps // 2))
    w = res["w"]
    terms = w["terms"]
    emit(what="Engine.waic, terms stored (integrate + accumulate + finish + results to the host)", rows=W, T=T,
         n_obs=n_obs, ms=round(ms_waic, 3), terms_GB=round(8.0 * n_obs * W / 1e9, 4), elpd_waic=w["summary"]["elpd_waic"],
         p_waic=w["summary"]["p_waic"], n_high_var=w["summary"]["n_high_var"])

    point = torch.empty((n_obs, len(N.LOO_POINT_FIELDS)), dtype=torch.float64, device=eng.dev)
    summary = torch.empty(len(N.LOO_SUMMARY_FIELDS), dtype=torch.float64, device=eng.dev)
    c = -(np.log(np.asarray(fp.obs_logsigma, dtype=float)) + 0.5 * np.log(2.0 * np.pi))
    eng._sync_stream()

    def loo_stage():
        eng.ctx.loo_run(terms.data_ptr(), n_obs, W, W, c, 1.0, point.data_ptr(), summary.data_ptr(), N.OE_ASYNC)

    ms_loo = timed(torch, loo_stage, a.reps)
    read_bytes = 8.0 * n_obs * W * (SELECT_PASSES + 1)
    sm = dict(zip(N.LOO_SUMMARY_FIELDS, summary.cpu().numpy().tolist()))
    pw = point.cpu().numpy()
    emit(what="oe_loo_run alone (6 x (k_loo_select + k_loo_pick), k_loo_gather + k_loo_merge, k_loo_fit, k_loo_finish)",
         rows=W, n_obs=n_obs, ms=round(ms_loo, 3), of_waic_pass=round(ms_loo / ms_waic, 3),
         read_GB=round(read_bytes / 1e9, 3), read_TBs=round(read_bytes / ms_loo / 1e9, 3),
         of_peak=round(read_bytes / ms_loo / 1e9 / PEAK_TBS, 3), n_tail_max=float(np.nanmax(pw[:, 5])),
         elpd_loo=sm["elpd_loo"], p_loo=sm["p_loo"], n_k_high=sm["n_k_high"], k_max=sm["k_max"])


if __name__ == "__main__":
    main()
