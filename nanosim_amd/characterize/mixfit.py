"""The error-length mixtures (src/model_fitting.py, F:27-217) are the fifth piece: the simulator does not start without
``<prefix>_model_profile``, which the reference fits to the three histograms ``hist()`` wrote — 512 + 9 216 + 9 216 Nelder-Mead searches
through scipy.  Here every search is one wavefront of one kernel (``ns_mixture_fit``; objective, evaluation order and search are written
down in csrc/ns_mixfit.h), three calls in all, and this module selects and writes as the reference does:

    characterize.model_fitting("training", eng)                             # reads training_{mis,ins,del}.hist -> training_model_profile

Deviations: a search whose residual is NaN never wins (the reference sorts its results with NaN among them, which leaves their order
undefined); a histogram that leaves no bin, or a type without a valid search, raises ValueError."""
import ctypes as C
import math

import numpy as np

from ._abi import arr, write_text


class NsMixfitFit(C.Structure):
    """mirror of ns_mixfit_fit (include/nanosim_amd.h)"""
    _fields_ = [("x", C.c_double * 4), ("fun", C.c_double), ("residual", C.c_double), ("nfev", C.c_uint32), ("nit", C.c_uint32),
                ("status", C.c_int32), ("reserved", C.c_uint32)]


class NsMixfitResult(C.Structure):
    """mirror of ns_mixfit_result (include/nanosim_amd.h)"""
    _fields_ = [("fits", C.c_void_p), ("ms_kernel", C.c_double)]


MIXFIT_DTYPE = np.dtype([("x", "<f8", (4,)), ("fun", "<f8"), ("residual", "<f8"), ("nfev", "<u4"), ("nit", "<u4"), ("status", "<i4"),
                         ("reserved", "<u4")])
MIXFIT_MISMATCH, MIXFIT_INDEL = 0, 1                        # NS_MIXFIT_*
MIXFIT_FIT, MIXFIT_EVALUATE = 0, 1
MIXFIT_TYPES = (("mis", "mismatch", "_mis.hist"), ("ins", "insertion", "_ins.hist"), ("del", "deletion", "_del.hist"))   # F:112-114, 136, 169, 203


def read_length_hist(path: str) -> dict:
    """{length: count} of a `_mis.hist` / `_ins.hist` / `_del.hist` file (F:28-33)"""
    h = {}
    with open(path) as f:
        f.readline()
        for line in f:
            info = line.strip().split()
            h[int(info[0])] = int(info[1])
    return h


def empirical_cdf(hist: dict, error: str):
    """(cdf, number of observations) as read_histogram (F:34-45) returns them for a {length: count} dict, without the list of
    observations: error "mis" — lengths shifted by one, max bins — or "indel" — max - 1 bins, so the last bin takes the two largest
    lengths.  np.histogram(density=True) divides by the bin width, which is 1 only when the smallest length present is the domain's
    first: kept.  A histogram that leaves no bin raises ValueError (numpy does in the reference)."""
    if error not in ("mis", "indel"):
        raise ValueError("error must be 'mis' or 'indel'")
    shift = 1 if error == "mis" else 0
    vals = sorted(k - shift for k, v in hist.items() if v > 0)
    if not vals:
        raise ValueError("empty histogram")
    bins = vals[-1] if error == "mis" else vals[-1] - 1
    if bins < 1:
        raise ValueError("the histogram leaves no bin (largest length %d)" % (vals[-1] + shift))
    w = np.array([hist[v + shift] for v in vals], dtype=np.float64)
    pmf, _ = np.histogram(np.array(vals, dtype=np.int64), bins=bins, weights=w, density=True)
    return np.cumsum(pmf), int(w.sum())


def fit_starts(error: str) -> np.ndarray:
    """the reference's grid of starts in its order: (512, 3) for "mis" (F:120-121), (9216, 4) for "indel" (F:153-154, 186-187) — whose
    tuples are built as (l, p, k, w) and read as (l, k, p, w) by ins_ll: kept, so column 1 runs over 0.1 .. 1.2 and column 2 over 0.1 .. 0.8"""
    a = np.arange
    if error == "mis":
        g = [(l, p, w) for l in a(0.1, 0.9, 0.1) for p in a(0.1, 0.9, 0.1) for w in a(0.1, 0.9, 0.1)]
    elif error == "indel":
        g = [(l, p, k, w) for l in a(0.1, 1.3, 0.1) for p in a(0.1, 1.3, 0.1) for k in a(0.1, 0.9, 0.1) for w in a(0.1, 0.9, 0.1)]
    else:
        raise ValueError("error must be 'mis' or 'indel'")
    return np.array(g, dtype=np.float64)


def mixture_fit(eng, error: str, cdf, starts, evaluate: bool = False) -> dict:
    """ns_mixture_fit: one Nelder-Mead search per start (or, with evaluate, the objective at each point).
    {"x": (n, 3 or 4), "fun", "residual", "nfev", "nit", "status": (n,), "ms_kernel"}"""
    dim = 3 if error == "mis" else 4
    cdf = arr(cdf, np.float64)
    starts = arr(starts, np.float64).reshape(-1, dim)
    fits = np.zeros(len(starts), dtype=MIXFIT_DTYPE)
    r = NsMixfitResult(fits=fits.ctypes.data)
    eng._check(eng.L.ns_mixture_fit(eng.ctx, MIXFIT_MISMATCH if error == "mis" else MIXFIT_INDEL, cdf.ctypes.data, len(cdf), starts.ctypes.data,
                                    len(starts), MIXFIT_EVALUATE if evaluate else MIXFIT_FIT, C.byref(r)))
    out = {k: fits[k].copy() for k in ("fun", "residual", "nfev", "nit", "status")}
    out["x"] = fits["x"][:, :dim].copy()
    out["ms_kernel"] = float(r.ms_kernel)
    return out


def select_fit(error: str, x, residual):
    """the index the reference's loop ends on (F:126-146, 160-179): the smallest residual whose parameters pass the validity test of
    F:131 / F:164, the earlier start on a tie (list.sort is stable); a NaN residual never wins.  None when no start qualifies."""
    x, residual = np.asarray(x), np.asarray(residual)
    if error == "mis":
        ok = (x[:, 0] > 0) & (x[:, 1] > 0) & (x[:, 1] < 1) & (x[:, 2] > 0) & (x[:, 2] < 1)
    else:
        ok = (x[:, 0] > 0) & (x[:, 1] > 0) & (x[:, 2] > 0) & (x[:, 2] < 1) & (x[:, 3] > 0) & (x[:, 3] < 1)
    ok &= ~np.isnan(residual)
    if not ok.any():
        return None
    r = np.where(ok, residual, np.inf)
    return int(np.argmin(r))                                # (the first of equal minima)


def fit_mixtures(eng, hists: dict) -> dict:
    """hists: {"mis" | "ins" | "del": {length: count}}.  Three calls of ns_mixture_fit over the reference's grids; per type
    {"params", "residual", "precision" = 1.36 / sqrt(n) (F:128), "warning": residual > precision (the reference's WARNING line), "start",
    "n_obs", "ms_kernel"}"""
    out = {}
    for t, _, _ in MIXFIT_TYPES:
        error = "mis" if t == "mis" else "indel"
        cdf, n_obs = empirical_cdf(hists[t], error)
        res = mixture_fit(eng, error, cdf, fit_starts(error))
        i = select_fit(error, res["x"], res["residual"])
        if i is None:
            raise ValueError("no search of the %s grid ended on valid parameters" % t)
        precision = 1.36 / math.sqrt(n_obs)
        out[t] = dict(params=[float(v) for v in res["x"][i]], residual=float(res["residual"][i]), precision=precision,
                      warning=bool(res["residual"][i] > precision), start=i, n_obs=n_obs, ms_kernel=res["ms_kernel"])
    return out


def format_model_profile(fit: dict) -> str:
    """the text of <prefix>_model_profile (F:110, 136, 169, 203): the mismatch row carries a literal 0 in the k column"""
    m, i, d = fit["mis"]["params"], fit["ins"]["params"], fit["del"]["params"]
    s = "Type\tlambda\tk\tprob\tweight\n"
    s += "mismatch\t" + str(m[0]) + '\t0\t' + str(m[1]) + '\t' + str(m[2]) + '\n'
    s += "insertion\t" + str(i[0]) + '\t' + str(i[1]) + '\t' + str(i[2]) + '\t' + str(i[3]) + '\n'
    s += "deletion\t" + str(d[0]) + '\t' + str(d[1]) + '\t' + str(d[2]) + '\t' + str(d[3]) + '\n'
    return s


def model_fitting(prefix: str, eng) -> dict:
    """model_fitting(prefix, threads) (F:108-217): reads <prefix>_mis.hist, _ins.hist and _del.hist as hist() wrote them and writes
    <prefix>_model_profile; returns fit_mixtures' dict"""
    fit = fit_mixtures(eng, {t: read_length_hist(prefix + suffix) for t, _, suffix in MIXFIT_TYPES})
    write_text(prefix + "_model_profile", format_model_profile(fit))
    return fit
