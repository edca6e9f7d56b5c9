"""GPU tests of the Sobol' sensitivity indices: the k_sobol_* kernels against
tests/sobol_ref.py, the estimator of include/odelib_amd.h (oe_sobol_begin) restated in numpy with
math.fsum for every sum.

Exact: n_V and every n_i; S1 == ST == 0.0 for a factor whose AB group is a bitwise copy of A;
NaN where the contract says NaN (no valid row, zero variance).
The cells (mean, M2, mx, my, M2x, M2y, Cxy): |Δ| <= C·unit + allowance, the units and the log
form's allowance as sobol_ref states them.  The constants C are 4 x the worst error measured on
the device in those units over every comparison of this file
(profiles/sobol/sobol_tolerances.log): measured worst mean 0.01639 (one ulp of
a mean of 63 values), M2 0.8371 (nb = 1: M2 of two values, under two ulp), Cxy 0.01154.  The
units grow with n, so the small cases set the constants.
S1, ST and V of k_sobol_finish: the contract's formulas in numpy on the device's own cells (the
blocks merged in block order by the same IEEE operations), to 8 ε of the larger operand; against
the reference, the cells' bounds propagated through the quotients."""
import ctypes as C
import math

import numpy as np
import pytest

import sobol_ref as R
from helpers import product_model
from odelib_amd import _native as N
from odelib_amd.engine import Engine, FitProblem, sobol_indices
from odelib_amd.Framework import band_inputs
from odelib_amd.Statistics import Samplers

pytestmark = pytest.mark.gpu

EPS = R.EPS
MEAN_WORST, M2_WORST, CXY_WORST = 0.01639, 0.8371, 0.01154
# 4 x the measured worst (module docstring)
CONST = {"mean": 4 * MEAN_WORST, "m2": 4 * M2_WORST, "cxy": 4 * CXY_WORST}
WORST, CASE = {}, {}
MASKS = [0b0111, 0b1000]


def _within(bad, group, name, got, want, unit, allowance=0.0):
    err = max(0.0, abs(got - want) - allowance)
    v = err / unit if unit > 0 else (0.0 if err == 0 else math.inf)
    WORST[group] = max(WORST.get(group, 0.0), v)
    CASE[group] = max(CASE.get(group, 0.0), v)
    if not v <= CONST[group]:
        bad.append((name, got, want, v, CONST[group]))


@pytest.fixture(scope="module")
def eng():
    """the oe_sobol_* calls need a context, not the problem in it"""
    e = Engine(FitProblem(model_id=N.OE_MODEL_TWO_I, n_states=4, n_params=5, times=np.linspace(0.0, 1.0, 5)))
    yield e
    e.close()


# ------------------------------------------------------------------ inputs
_MADE = {}


def make(nb, d):
    """values [3][4][(d + 2) nb], group-major.  The states are log-normal responses to d factors,
    so the indices are spread over (0, 1).  Row 1 is the constant 2.5 (V == 0).  Row 2: the last
    factor's group is a bitwise copy of A, and state 3 (column 1) has no valid value at all.
    Row 0 (nb >= 16): NaN, inf, 0 and negative values planted in an A value only, a B value only
    and one AB_0 value only (0 and the negatives count in the identity form alone)."""
    if (nb, d) in _MADE:
        return _MADE[(nb, d)]
    rs = np.random.RandomState(100 * d + nb % 97)
    G = d + 2
    xa, xb = rs.standard_normal((nb, d)), rs.standard_normal((nb, d))
    w = rs.uniform(0.2, 1.0, size=(3, 4, d))
    v = np.empty((3, 4, G, nb))
    for g in range(G):
        x = xa.copy() if g != 1 else xb
        if g >= 2:
            x[:, g - 2] = xb[:, g - 2]
        v[:, :, g, :] = np.exp(10.0 + 0.3 * np.einsum("tsd,nd->tsn", w, x) + 0.1 * np.sin(3.0 * x.sum(axis=1)))
    v[1] = 2.5
    v[2, :, G - 1, :] = v[2, :, 0, :]
    v[2, 3] = np.nan
    if nb >= 16:
        v[0, 3, 0, 1] = np.nan
        v[0, 3, 0, 2] = 0.0
        v[0, 1, 0, 4] = np.nan     # column 0 = states 0 + 1 + 2
        v[0, 3, 1, 5] = np.inf
        v[0, 3, 1, 6] = -3.0
        v[0, 0, 1, 7] = -np.inf
        v[0, 3, 2, 9] = np.nan
        v[0, 3, 2, 10] = -1e-3
        v[0, 2, 2, 11] = np.inf
    out = np.ascontiguousarray(v.reshape(3, 4, G * nb))
    out.setflags(write=False)
    _MADE[(nb, d)] = out
    return out


_REFS = {}


def ref_of(nb, d, log, rows=None):
    key = (nb, d, log, None if rows is None else (rows.start, rows.stop))
    if key not in _REFS:
        _REFS[key] = R.reference(make(nb, d), MASKS, d, log, rows)
    return _REFS[key]


def chunk_of(values, G, a, b):
    """base rows [a, b) of a group-major tensor, as a chunk of its own"""
    T, S, W = values.shape
    return np.ascontiguousarray(values.reshape(T, S, G, W // G)[..., a:b].reshape(T, S, G * (b - a)))


def run(eng, values, masks, d, log, blocks=1, splits=None):
    """the three calls on a host tensor: ``splits`` the chunk sizes of every block (default: one
    chunk).  Returns (acc [R][T][C][cell], idx [T][C][d][3], out [T][C][3])."""
    torch = eng.torch
    T, S, W = values.shape
    G = d + 2
    n_base = W // G
    per = n_base // blocks
    assert per * blocks == n_base
    splits = [per] if splits is None else splits
    assert sum(splits) == per
    f64 = torch.float64
    cell = N.sobol_cell(d)
    acc = torch.full((blocks, T, len(masks), cell), -7.0, dtype=f64, device=eng.dev)
    idx = torch.empty((T, len(masks), d, 3), dtype=f64, device=eng.dev)
    out = torch.empty((T, len(masks), 3), dtype=f64, device=eng.dev)
    eng._sync_stream()
    args = eng.ctx.sobol_args(T, S, masks, d, n_base, log, blocks)
    eng.ctx.sobol_begin(args, C.c_void_p(acc.data_ptr()), N.OE_ASYNC)
    for r in range(blocks):
        a = r * per
        for n in splits:
            t = torch.as_tensor(chunk_of(values, G, a, a + n).copy(), device=eng.dev)
            eng.ctx.sobol_accum(args, r, n, C.c_void_p(t.data_ptr()), C.c_void_p(acc.data_ptr()), N.OE_ASYNC)
            a += n
    eng.ctx.sobol_finish(args, C.c_void_p(acc.data_ptr()), C.c_void_p(idx.data_ptr()), C.c_void_p(out.data_ptr()))
    return acc.cpu().numpy(), idx.cpu().numpy(), out.cpu().numpy()


# ------------------------------------------------------------------ checks
def check_cells(cells, ref, d, label):
    """one block's cells [T][C][cell] against the reference: counts exact, floats within bounds"""
    bad = []
    CASE.clear()
    for t, row in enumerate(ref):
        for c, r in enumerate(row):
            at = (label, t, c)
            got = cells[t, c]
            assert got[0] == r["n_valid"], at
            if r["n_valid"]:
                _within(bad, "mean", at + ("mean",), got[1], r["mean"], r["u_mean"], r["a_mean"])
                _within(bad, "m2", at + ("m2",), got[2], r["m2"], r["u_m2"], r["a_m2"])
            for i, f in enumerate(r["factors"]):
                g = got[3 + 6 * i:9 + 6 * i]
                assert g[0] == f["n"], at + (i,)
                if not f["n"]:
                    continue
                _within(bad, "mean", at + (i, "mx"), g[1], f["mx"], f["u_mx"], f["a_mx"])
                _within(bad, "mean", at + (i, "my"), g[2], f["my"], f["u_my"], f["a_my"])
                _within(bad, "m2", at + (i, "m2x"), g[3], f["m2x"], f["u_m2x"], f["a_m2x"])
                _within(bad, "m2", at + (i, "m2y"), g[4], f["m2y"], f["u_m2y"], f["a_m2y"])
                _within(bad, "cxy", at + (i, "cxy"), g[5], f["cxy"], f["u_cxy"], f["a_cxy"])
    print(f"sobol cells {label}: worst error in units of the bounds: mean {CASE.get('mean', 0):.3g}, "
          f"M2 {CASE.get('m2', 0):.3g}, Cxy {CASE.get('cxy', 0):.3g}")
    assert not bad, bad[:5]


def index_bounds(r, f):
    """the cells' bounds propagated to V, S1 and ST (first order, plus 8 ε for the quotients)"""
    nv, n = r["n_valid"], f["n"]
    b_m2 = CONST["m2"] * r["u_m2"] + r["a_m2"]
    rel_v = b_m2 / r["m2"] + 8 * EPS
    b_cxy = CONST["cxy"] * f["u_cxy"] + f["a_cxy"]
    b_m2y = CONST["m2"] * f["u_m2y"] + f["a_m2y"]
    b_my = CONST["mean"] * f["u_my"] + f["a_my"]
    V = r["m2"] / nv
    s1 = b_cxy / n / V + abs(f["S1"]) * rel_v
    st = (b_m2y / n + 2 * abs(f["my"]) * b_my + b_my * b_my) / 2 / V + abs(f["ST"]) * rel_v
    return s1, st


def check_indices(idx, out, ref, label):
    """k_sobol_finish's outputs against the reference"""
    for t, row in enumerate(ref):
        for c, r in enumerate(row):
            at = (label, t, c)
            assert out[t, c, 0] == r["n_valid"], at
            if not r["n_valid"]:
                assert np.isnan(out[t, c, 1]) and np.isnan(out[t, c, 2]), at
            else:
                assert abs(out[t, c, 2] - r["var"]) <= (CONST["m2"] * r["u_m2"] + r["a_m2"]) / r["n_valid"] \
                    + 8 * EPS * r["var"], at
            for i, f in enumerate(r["factors"]):
                assert idx[t, c, i, 2] == f["n"], at + (i,)
                if not (r["n_valid"] and r["var"] > 0 and f["n"]):
                    assert np.isnan(idx[t, c, i, 0]) and np.isnan(idx[t, c, i, 1]), at + (i,)
                    continue
                b1, bt = index_bounds(r, f)
                assert abs(idx[t, c, i, 0] - f["S1"]) <= b1, at + (i, "S1", idx[t, c, i, 0], f["S1"], b1)
                assert abs(idx[t, c, i, 1] - f["ST"]) <= bt, at + (i, "ST", idx[t, c, i, 1], f["ST"], bt)
                assert idx[t, c, i, 1] >= 0.0, at + (i,)


def merge_blocks(acc, d):
    """the blocks' cells [R][...][cell] merged in block order from the empty cell, with reduce.cuh's
    Chan merges restated operation by operation"""
    def pick(be, ae, a, b, m):
        return np.where(be, a, np.where(ae, b, m))

    shape = acc.shape[1:-1]
    var = [np.zeros(shape) for _ in range(3)]
    cov = [[np.zeros(shape) for _ in range(6)] for _ in range(d)]
    with np.errstate(all="ignore"):
        for r in range(acc.shape[0]):
            bn, bm, b2 = (acc[r, ..., k] for k in range(3))
            an, am, a2 = var
            n = an + bn
            dl = bm - am
            rb = bn / n
            ae, be = an == 0, bn == 0
            var = [n, pick(be, ae, am, bm, am + dl * rb), pick(be, ae, a2, b2, (a2 + b2) + (dl * dl) * (an * rb))]
            for i in range(d):
                b = [acc[r, ..., 3 + 6 * i + k] for k in range(6)]
                a = cov[i]
                n = a[0] + b[0]
                dx, dy = b[1] - a[1], b[2] - a[2]
                rb = b[0] / n
                f = a[0] * rb
                ae, be = a[0] == 0, b[0] == 0
                cov[i] = [n, pick(be, ae, a[1], b[1], a[1] + dx * rb), pick(be, ae, a[2], b[2], a[2] + dy * rb),
                          pick(be, ae, a[3], b[3], (a[3] + b[3]) + (dx * dx) * f),
                          pick(be, ae, a[4], b[4], (a[4] + b[4]) + (dy * dy) * f),
                          pick(be, ae, a[5], b[5], (a[5] + b[5]) + (dx * dy) * f)]
    return np.stack(var + [x for cv in cov for x in cv], axis=-1)


def check_finish(acc, idx, out, d, label):
    """S1, ST, V are the contract's formulas on the device's own cells, to 8 ε of the larger operand"""
    cells = merge_blocks(acc, d)
    want = sobol_indices(cells, d)
    cov = cells[..., 3:].reshape(cells.shape[:-1] + (d, 6))

    def same(got, ref, scale, what):
        both_nan = np.isnan(got) & np.isnan(ref)
        with np.errstate(invalid="ignore"):
            ok = both_nan | (np.abs(got - ref) <= 8 * EPS * scale)
        assert ok.all(), (label, what, np.argwhere(~ok)[:3], got[~ok][:3], ref[~ok][:3])

    assert np.array_equal(out[..., 0], cells[..., 0]) and np.array_equal(idx[..., 2], cov[..., 0]), label
    with np.errstate(all="ignore"):
        V = want["var"]
        same(out[..., 2], V, np.abs(V), "V")
        same(out[..., 1], want["mean"], np.abs(want["mean"]), "mean")
        same(idx[..., 0], want["S1"], np.abs(want["S1"]), "S1")
        larger = np.maximum(cov[..., 4] / cov[..., 0], cov[..., 2] ** 2) / 2 / V[..., None]
        same(idx[..., 1], want["ST"], np.maximum(np.abs(want["ST"]), larger), "ST")


# ------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("log", [True, False], ids=["log", "identity"])
@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("nb", [1, 63, 257, 3000])
def test_kernels_against_the_reference(eng, nb, d, log):
    values = make(nb, d)
    acc, idx, out = run(eng, values, MASKS, d, log)
    assert (acc != -7.0).all()  # k_sobol_init and the merges wrote every double
    ref = ref_of(nb, d, log)
    label = f"nb={nb} d={d} {'log' if log else 'identity'}"
    check_cells(acc[0], ref, d, label)
    check_indices(idx, out, ref, label)
    check_finish(acc, idx, out, d, label)
    # the constant row: full counts, zero variance, NaN indices
    assert (out[1, :, 0] == 2 * nb).all() and (out[1, :, 2] == 0.0).all() and np.isnan(idx[1, :, :, :2]).all()
    assert (idx[1, :, :, 2] == nb).all()
    # the cell without a valid value
    assert out[2, 1, 0] == 0 and np.isnan(out[2, 1, 1:]).all() and np.isnan(idx[2, 1, :, :2]).all()
    assert (idx[2, 1, :, 2] == 0).all()
    # the copied group
    assert idx[2, 0, d - 1, 0] == 0.0 and idx[2, 0, d - 1, 1] == 0.0, idx[2, 0, d - 1]
    assert out[2, 0, 2] > 0 and idx[2, 0, d - 1, 2] == nb
    if nb >= 16:  # what the plants dropped, per factor
        drop_a, drop_b = (2, 2) if log else (1, 1)
        assert out[0, 1, 0] == 2 * (nb - drop_a - drop_b)
        assert idx[0, 1, 0, 2] == nb - drop_a - drop_b - (2 if log else 1)
        if d > 1:
            assert idx[0, 1, 1, 2] == nb - drop_a - drop_b
        assert out[0, 0, 0] == 2 * (nb - 2) and idx[0, 0, 0, 2] == nb - 3


@pytest.mark.parametrize("log", [True, False], ids=["log", "identity"])
def test_chunking_and_blocks(eng, log):
    nb, d = 3000, 5
    values = make(nb, d)
    ref = ref_of(nb, d, log)
    one = run(eng, values, MASKS, d, log)
    again = run(eng, values, MASKS, d, log)
    for a, b in zip(one, again):
        assert a.tobytes() == b.tobytes()  # two identical runs: identical bits
    three = run(eng, values, MASKS, d, log, splits=[1024, 1024, 952])
    assert three[0].tobytes() == run(eng, values, MASKS, d, log, splits=[1024, 1024, 952])[0].tobytes()
    assert np.array_equal(three[0][..., 0], one[0][..., 0]) and np.array_equal(three[1][..., 2], one[1][..., 2])
    check_cells(three[0][0], ref, d, f"three chunks {'log' if log else 'identity'}")
    check_indices(three[1], three[2], ref, "three chunks")
    assert np.isnan(engine_se(one[0], d)).all()
    for splits in (None, [256, 256, 238]):
        acc, idx, out = run(eng, values, MASKS, d, log, blocks=4, splits=splits)
        label = f"4 blocks {splits} {'log' if log else 'identity'}"
        for r in range(4):  # each block's cells against the reference of its own base rows
            check_cells(acc[r], ref_of(nb, d, log, slice(750 * r, 750 * (r + 1))), d, f"{label} block {r}")
        assert np.array_equal(out[..., 0], one[2][..., 0]) and np.array_equal(idx[..., 2], one[1][..., 2])
        check_indices(idx, out, ref, label)  # the pooled result, within the 1-block result's bounds
        check_finish(acc, idx, out, d, label)
        se = engine_se(acc, d)
        ok = ~np.isnan(idx[..., :2])
        assert np.isfinite(se[ok]).all() and (se[ok] >= 0).all(), label
        assert np.isfinite(se[0, 0]).all()


def engine_se(acc, d):
    from odelib_amd.engine import sobol_se
    s1, st = sobol_se(acc, d)
    return np.stack([s1, st], axis=-1)


# ------------------------------------------------------------------ a function with known indices
def test_ishigami_analytic(eng):
    import scipy.stats
    from odelib_amd import parameter
    pr = {k: parameter(stats_gen=scipy.stats.uniform, hyperparameters={"loc": -math.pi, "scale": 2 * math.pi},
                       init_value=1.0) for k in ("x1", "x2", "x3")}
    A, B = (f.to_numpy() for f in Samplers.sample_saltelli(pr, 4096, seed=0))
    groups = [A, B]
    for i in range(3):
        AB = A.copy()
        AB[:, i] = B[:, i]
        groups.append(AB)
    values = np.concatenate([R.ishigami(g) for g in groups]).reshape(1, 1, -1)
    assert values.shape[2] == 20480
    acc, idx, out = run(eng, values, [1], 3, False, blocks=8)
    print("ishigami on the device: S1", idx[0, 0, :, 0], "ST", idx[0, 0, :, 1])
    assert np.abs(idx[0, 0, :, 0] - np.array(R.ISHIGAMI_S1)).max() < 0.01
    assert np.abs(idx[0, 0, :, 1] - np.array(R.ISHIGAMI_ST)).max() < 0.01
    ref = R.reference(values, [1], 3, False)
    check_indices(idx, out, ref, "ishigami")
    check_finish(acc, idx, out, 3, "ishigami")
    for r in range(8):
        check_cells(acc[r], R.reference(values, [1], 3, False, slice(512 * r, 512 * (r + 1))), 3, f"ishigami block {r}")
    assert np.isfinite(engine_se(acc, 3)).all()


# ------------------------------------------------------------------ end to end
def design_chunks(m, drawn, n_base, seed, blocks, chunk):
    """The walkers of ModelFramework.sobol's design, chunk by chunk as Engine.sobol lays them out:
    (theta [P][G nb], y0 [S][G nb]) per chunk."""
    pn, sn = m.get_pnames(), list(m._snames)
    fa, fb = Samplers.sample_saltelli(drawn, n_base, seed)
    for frame in (fa, fb):
        for p in pn:
            if p not in drawn:
                frame[p] = float(np.asarray(m.parameters[p].val))
    (ta, ya), (tb, yb) = band_inputs(pn, sn, m.get_inits(), fa), band_inputs(pn, sn, m.get_inits(), fb)
    per = n_base // blocks
    out = []
    for r in range(blocks):
        for a in range(r * per, (r + 1) * per, chunk):
            b = min(a + chunk, (r + 1) * per)
            th, y0 = [ta[:, a:b], tb[:, a:b]], [ya[:, a:b], yb[:, a:b]]
            for p in drawn:
                t = ta[:, a:b].copy()
                t[pn.index(p)] = tb[pn.index(p), a:b]
                th.append(t)
                y0.append(ya[:, a:b])  # (no '<state>0' factor in these tests)
            out.append((np.concatenate(th, axis=1), np.concatenate(y0, axis=1), b - a))
    return out


@pytest.mark.parametrize("method", ["rk4", None], ids=["rk4", "default"])
def test_model_framework_sobol_end_to_end(method):
    kw = {} if method is None else {"method": method}
    m = product_model("two_i", extra_params={"zz": 1.0}, **kw)
    ranges = {"zz": (0.5, 2.0)}
    n_base, blocks, chunk, seed = 512, 4, 64, 0
    long, chi = m.sobol(n_base=n_base, ranges=ranges, seed=seed, log=True, blocks=blocks, chunk=chunk)
    drawn = m._sobol_factors(None, ranges)
    fnames = list(drawn)
    d, G = len(fnames), len(fnames) + 2
    assert fnames == ["mu", "phi", "beta", "lam", "tau", "zz"]
    names = m.get_snames(after_summation=True)
    T = len(m.times)
    assert list(long.columns) == ["time", "organism", "parameter", "S1", "ST", "S1_se", "ST_se", "n"]
    assert len(long) == T * len(names) * d and list(chi["parameter"]) == fnames
    assert "status_or" in long.attrs and "n_status" in chi.attrs
    # the engine's own trajectories and chi of the same walkers in the same launches' layout
    groups_t = [[] for _ in range(G)]
    groups_c = [[] for _ in range(G)]
    for th, y0, nb in design_chunks(m, drawn, n_base, seed, blocks, chunk):
        res = m.integrate_batch(th.T, inits=y0.T)
        tr, ch = res["traj"].cpu().numpy(), res["chi"].cpu().numpy()
        for g in range(G):
            groups_t[g].append(tr[:, :, g * nb:(g + 1) * nb])
            groups_c[g].append(ch[g * nb:(g + 1) * nb])
    values = np.concatenate([np.concatenate(g, axis=2) for g in groups_t], axis=2)
    chis = np.concatenate([np.concatenate(g) for g in groups_c]).reshape(1, 1, -1)
    masks = [int(v) for v in m._band_masks()]
    # every grid row: the device's n_V and n_i against the counts of the engine's own trajectories
    ok_all = R.outputs(R.columns(values, masks), True)[1]
    ok_all = ok_all.reshape(T, len(masks), G, n_base)
    both = ok_all[:, :, 0] & ok_all[:, :, 1]
    got = {k: np.transpose(long[k].to_numpy().reshape(len(names), d, T), (2, 0, 1)) for k in ("S1", "ST", "n", "S1_se")}
    assert np.array_equal(long.attrs["n_valid"], 2 * both.sum(-1))
    assert np.array_equal(got["n"], (both[:, :, None] & ok_all[:, :, 2:]).sum(-1))
    # the fsum reference on a spread of grid rows, both ends included (every row runs the same code;
    # all 1000 rows of it take 5 s): the device's mean and V, and S1 and ST, within the bounds
    sel = sorted(set([0, 1, 2, T - 1] + list(range(5, T, 40))))
    ref = R.reference(values[sel], masks, d, True)
    ref_chi = R.reference(chis, [1], d, False)
    idx = np.stack([got["S1"], got["ST"], got["n"].astype(float)], axis=-1)[sel]
    out = np.stack([long.attrs["n_valid"].astype(float), long.attrs["mean"], long.attrs["var"]], axis=-1)[sel]
    bad = []
    for t, row in enumerate(ref):
        for c, r in enumerate(row):
            _within(bad, "mean", (method, sel[t], c, "mean"), out[t, c, 1], r["mean"], r["u_mean"], r["a_mean"])
    assert not bad, bad[:5]
    check_indices(idx, out, ref, f"two_i {method}")
    idx_chi = np.stack([chi["S1"].to_numpy(), chi["ST"].to_numpy(), chi["n"].to_numpy().astype(float)], axis=-1)[None, None]
    out_chi = np.array([[[ref_chi[0][0]["n_valid"], chi.attrs["mean"], chi.attrs["var"]]]])
    assert chi.attrs["n_valid"] == ref_chi[0][0]["n_valid"]
    check_indices(idx_chi, out_chi, ref_chi, f"two_i chi {method}")
    # grid row 0: every walker starts alike
    assert np.isnan(got["S1"][0]).all() and np.isnan(got["ST"][0]).all()
    defined = ~np.isnan(got["ST"])
    assert defined[1:].all() and (got["ST"][defined] >= 0).all()
    assert np.isfinite(got["S1_se"][1:]).all()
    if method == "rk4":  # a factor the right-hand side never reads: exactly no effect
        z = fnames.index("zz")
        assert (got["S1"][1:, :, z] == 0.0).all() and (got["ST"][1:, :, z] == 0.0).all()
        assert chi["S1"][z] == 0.0 and chi["ST"][z] == 0.0
        assert (np.abs(got["ST"][1:, :, :z]).max(axis=(0, 1)) > 1e-6).all()  # the others do move the states


# ------------------------------------------------------------------ C-ABI errors
def test_c_abi_errors_are_codes_and_launch_nothing(eng):
    torch = eng.torch
    lib, h = eng.ctx.lib, eng.ctx._h
    d = 2
    acc = torch.full((2, 3, 2, N.sobol_cell(d)), -7.0, dtype=torch.float64, device=eng.dev)
    vals = torch.ones((3, 4, 4 * 8), dtype=torch.float64, device=eng.dev)
    idx = torch.full((3, 2, d, 3), -7.0, dtype=torch.float64, device=eng.dev)
    out = torch.full((3, 2, 3), -7.0, dtype=torch.float64, device=eng.dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def args(**kw):
        base = dict(n_rows=3, n_states=4, col_masks=MASKS, n_factors=d, n_base=8, log_form=True, n_blocks=2)
        base.update(kw)
        return eng.ctx.sobol_args(**base)

    def all_three(a, code, word):
        for rc in (lib.oe_sobol_begin(h, C.byref(a), p(acc), 0), lib.oe_sobol_accum(h, C.byref(a), 0, 8, p(vals), p(acc), 0),
                   lib.oe_sobol_finish(h, C.byref(a), p(acc), p(idx), p(out), 0)):
            assert rc == code
            assert word in lib.oe_last_error(h).decode(), lib.oe_last_error(h)

    ok = args()
    all_three(args(n_factors=0), N.OE_ERR_ARG, "n_factors")
    all_three(args(n_factors=33), N.OE_ERR_ARG, "n_factors")
    all_three(args(col_masks=[1] * 65), N.OE_ERR_ARG, "n_cols")
    all_three(args(col_masks=[0b0111, 0]), N.OE_ERR_ARG, "col_mask")
    all_three(args(col_masks=[0b10000]), N.OE_ERR_ARG, "col_mask")
    all_three(args(n_blocks=0), N.OE_ERR_ARG, "n_blocks")
    all_three(args(n_base=0), N.OE_ERR_ARG, "n_base")
    all_three(args(n_base=(1 << 29) // 4 + 1), N.OE_ERR_ARG, "n_base")
    nomask = args()
    nomask.col_mask = None
    all_three(nomask, N.OE_ERR_ARG, "col_mask")
    # null pointers, host pointers, a null struct
    assert lib.oe_sobol_begin(h, C.byref(ok), None, 0) == N.OE_ERR_ARG and b"acc" in lib.oe_last_error(h)
    assert lib.oe_sobol_accum(h, C.byref(ok), 0, 8, None, p(acc), 0) == N.OE_ERR_ARG and b"values" in lib.oe_last_error(h)
    assert lib.oe_sobol_accum(h, C.byref(ok), 0, 8, p(vals), None, 0) == N.OE_ERR_ARG
    assert lib.oe_sobol_finish(h, C.byref(ok), p(acc), None, p(out), 0) == N.OE_ERR_ARG and b"idx" in lib.oe_last_error(h)
    assert lib.oe_sobol_finish(h, C.byref(ok), None, p(idx), p(out), 0) == N.OE_ERR_ARG
    assert lib.oe_sobol_finish(h, C.byref(ok), p(acc), p(idx), None, 0) == N.OE_ERR_ARG
    assert lib.oe_sobol_begin(h, None, p(acc), 0) == N.OE_ERR_ARG and b"args" in lib.oe_last_error(h)
    assert lib.oe_sobol_begin(h, C.byref(ok), p(acc), N.OE_HOST_PTRS) == N.OE_ERR_ARG
    assert b"device pointers" in lib.oe_last_error(h)
    assert lib.oe_sobol_accum(h, C.byref(ok), 0, 8, p(vals), p(acc), N.OE_HOST_PTRS) == N.OE_ERR_ARG
    assert lib.oe_sobol_finish(h, C.byref(ok), p(acc), p(idx), p(out), N.OE_HOST_PTRS) == N.OE_ERR_ARG
    assert lib.oe_sobol_accum(h, C.byref(ok), 2, 8, p(vals), p(acc), 0) == N.OE_ERR_ARG and b"block" in lib.oe_last_error(h)
    assert lib.oe_sobol_accum(h, C.byref(ok), 0, 9, p(vals), p(acc), 0) == N.OE_ERR_ARG and b"nb" in lib.oe_last_error(h)
    assert lib.oe_sobol_accum(h, C.byref(ok), 0, 0, p(vals), p(acc), 0) == N.OE_ERR_ARG
    assert lib.oe_sobol_begin(None, C.byref(ok), p(acc), 0) == N.OE_ERR_STATE
    torch.cuda.synchronize(eng.dev)
    for t in (acc, idx, out):  # nothing was launched
        assert (t == -7.0).all()
    # and the same arguments, valid, do run
    assert lib.oe_sobol_begin(h, C.byref(ok), p(acc), 0) == N.OE_OK
    assert (acc == 0.0).all()


def test_zz_report_worst_errors():
    """(last in the file) the worst error of each kind over every comparison above, in its unit"""
    print("sobol worst errors over this file's comparisons, in units of the bounds:",
          ", ".join(f"{k} {v:.4g} (constant {CONST[k]:.4g})" for k, v in sorted(WORST.items())))
