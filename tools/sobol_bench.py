"""Sobol' sensitivity reduction on two_i, T = 1000, d = 5 factors (G = 7 groups) and the largest
chunk the 1 GiB budget allows (4608 base rows, 32 256 walkers, a 1.03 GB trajectory chunk).

Times, after >= 60 ms of warm-up launches, k_sobol_accum + k_sobol_merge on that chunk (log and
identity form); the existing k_band_moments + k_band_merge pass over the same bytes as the
yardstick; the estimator written with torch on the same device; and ModelFramework.sobol end to
end.  ``--variants name=path,...`` repeats the kernel timings in a fresh process per library
(builds of csrc with another OE_SOBOL_FACTOR_TILE).  Bytes: ``chunk`` is the trajectory chunk read
once; ``requested`` counts A and B once per factor tile, as the kernel asks for them.  Prints one
JSON line per measurement; recorded in DESIGN.md §3.15 and profiles/sobol/, not gated.

    python tools/sobol_bench.py [--reps 10] [--big 131072] [--kernels-only] [--variants pt1=...,pt4=...]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--big", type=int, default=131072)
    ap.add_argument("--tile", type=int, default=0, help="the library's factor tile, for the requested bytes (0: the source's)")
    ap.add_argument("--kernels-only", action="store_true", help="skip the torch baseline and the end-to-end runs")
    ap.add_argument("--variants", default="", help="name=library,...: the kernel timings again, one fresh process each")
    ap.add_argument("--wg", default="", help="workgroups per CU, e.g. 2,4,8,16: the kernel timings again, one fresh process each")
    ap.add_argument("--label", default="default")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import _demo_problem
    from odelib_amd import _native as N
    from odelib_amd.engine import sobol_chunk, sobol_indices

    tile = a.tile
    if not tile:
        import re
        src = open(os.path.join(ROOT, "odelib_amd", "csrc", "sobol.cuh")).read()
        tile = int(re.search(r"#define OE_SOBOL_FACTOR_TILE (\d+)", src).group(1))

    m, th = _demo_problem("rk4")
    eng = m.engine()
    T, S, d = len(m.times), 4, len(th)
    G = d + 2
    nb = sobol_chunk(T, S, G)
    W = G * nb
    masks = m._band_masks()
    rs = np.random.RandomState(0)
    ta = (th[None, :] * np.exp(0.05 * rs.standard_normal((nb, d)))).T
    tb = (th[None, :] * np.exp(0.05 * rs.standard_normal((nb, d)))).T
    groups = [ta, tb]
    for i in range(d):
        t = ta.copy()
        t[i] = tb[i]
        groups.append(t)
    theta = np.ascontiguousarray(np.concatenate(groups, axis=1))
    y0 = np.repeat(np.asarray(m.get_inits(), float)[:, None], W, axis=1)
    chunk_bytes = 8.0 * S * T * W
    tiles = -(-d // tile)
    requested = 8.0 * S * T * nb * (d + 2 * tiles)
    traj = eng.empty_traj(W)
    eng.integrate(y0, theta, traj_out=traj)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def emit(**kw):
        print(json.dumps(dict(lib=a.label, wg_per_cu=os.environ.get("OE_SOBOL_WG_PER_CU", "default"), **kw)), flush=True)

    cell = N.sobol_cell(d)
    acc = torch.empty((1, T, len(masks), cell), dtype=torch.float64, device=eng.dev)
    idx = torch.empty((T, len(masks), d, 3), dtype=torch.float64, device=eng.dev)
    out = torch.empty((T, len(masks), 3), dtype=torch.float64, device=eng.dev)
    res = {}
    for log in (True, False):
        args = eng.ctx.sobol_args(T, S, masks, d, nb, log, 1)
        eng.ctx.sobol_begin(args, P(acc))
        eng.ctx.sobol_accum(args, 0, nb, P(traj), P(acc))
        eng.ctx.sobol_finish(args, P(acc), P(idx), P(out))
        res[log] = idx.cpu().numpy().copy()
        ms = timed(torch, lambda: eng.ctx.sobol_accum(args, 0, nb, P(traj), P(acc), N.OE_ASYNC), a.reps)
        emit(what="k_sobol_accum+k_sobol_merge", form="log" if log else "identity", factor_tile=tile, base_rows=nb, walkers=W,
             T=T, d=d, ms=round(ms, 4), chunk_GB=round(chunk_bytes / 1e9, 4), chunk_read_TBs=round(chunk_bytes / ms / 1e9, 3),
             chunk_of_peak=round(chunk_bytes / ms / 1e9 / PEAK_TBS, 3), requested_GB=round(requested / 1e9, 4),
             requested_TBs=round(requested / ms / 1e9, 3))
    bacc = torch.empty((T, len(masks), 5), dtype=torch.float64, device=eng.dev)
    bhist = torch.empty((T, len(masks), 1024), dtype=torch.int32, device=eng.dev)
    eng.ctx.band_begin(masks, 1024, P(bacc), P(bhist))
    ms = timed(torch, lambda: eng.ctx.band_moments(W, P(traj), P(bacc), N.OE_ASYNC), a.reps)
    emit(what="k_band_moments+k_band_merge on the same chunk (the yardstick)", walkers=W, T=T, ms=round(ms, 4),
         chunk_read_TBs=round(chunk_bytes / ms / 1e9, 3), chunk_of_peak=round(chunk_bytes / ms / 1e9 / PEAK_TBS, 3))
    if a.kernels_only:
        return

    sel = [torch.tensor([s for s in range(S) if (int(k) >> s) & 1], device=eng.dev) for k in masks]

    def torch_sobol():
        """the estimator with torch: every row valid (true of this chunk), centred as the contract"""
        f = torch.stack([traj[:, ix].sum(1) for ix in sel], dim=1).log().view(T, len(masks), G, nb)
        fa, fb, fab = f[:, :, 0], f[:, :, 1], f[:, :, 2:]
        V = torch.cat([fa, fb], dim=-1).var(-1, unbiased=False)
        y = fab - fa[:, :, None]
        xc = fb - fb.mean(-1, keepdim=True)
        s1 = (xc[:, :, None] * (y - y.mean(-1, keepdim=True))).mean(-1) / V[..., None]
        st = (y * y).mean(-1) / 2 / V[..., None]
        return s1, st

    s1, st = (t.cpu().numpy() for t in torch_sobol())
    tms = timed(torch, torch_sobol, max(2, a.reps // 3))
    with np.errstate(invalid="ignore"):
        emit(what="torch: the same estimator (sum, log, var, centred products; no validity, no blocks)", walkers=W, T=T,
             ms=round(tms, 4), chunk_read_TBs=round(chunk_bytes / tms / 1e9, 3),
             S1_max_abs_diff=float(np.nanmax(np.abs(s1 - res[True][..., 0]))),
             ST_max_abs_diff=float(np.nanmax(np.abs(st - res[True][..., 1]))))
    del traj, acc, bacc, bhist
    torch.cuda.empty_cache()

    ranges = {p: (0.8 * v, 1.25 * v) for p, v in zip(m.get_pnames(), th)}
    m.sobol(n_base=512, ranges=ranges, blocks=8)  # warm
    for n_base in (8192, a.big):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        long, chi = m.sobol(n_base=n_base, ranges=ranges, blocks=8)
        dt = time.perf_counter() - t0
        last = long[long["time"] == long["time"].max()]
        emit(what="ModelFramework.sobol end to end", n_base=n_base, walkers=n_base * G, T=T, seconds=round(dt, 4),
             n_min=int(long["n"].min()), n_status=int(long.attrs["n_status"]),
             ST_V_at_the_end={r.parameter: round(float(r.ST), 4) for r in last[last["organism"] == "V"].itertuples()},
             ST_chi={r.parameter: round(float(r.ST), 4) for r in chi.itertuples()})

    for item in filter(None, a.variants.split(",")):  # a fresh process each: the library is loaded once
        name, path = item.split("=", 1)
        env = dict(os.environ, ODELIB_AMD_LIB=os.path.abspath(path))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--reps", str(a.reps), "--label", name,
                        "--tile", name.lstrip("pt")], env=env, check=True, timeout=300)
    for wg in filter(None, a.wg.split(",")):  # the library reads the variable once
        env = dict(os.environ, OE_SOBOL_WG_PER_CU=wg)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--reps", str(a.reps)], env=env,
                       check=True, timeout=300)


if __name__ == "__main__":
    main()

