"""The producer/consumer moment kernel (k_moments_ws) at the smallest shapes where its tile
pipeline, its instances and its phasor fix-up can go wrong.

Two checks per case, on harmonic fits:

(1) the records are those of the parent build, bit for bit: sha256 of the record array against
    tests/golden/moments_parent_records.json, recorded on the GPU from the commit before the
    moment kernel's instruction stream was taken in hand (its build id is in the file; `python
    tests/test_gpu_moments_schedule.py FILE` records a new set from the library in the tree).
    The kernel's arithmetic is meant to stay the same operation by operation, so nothing here
    has a tolerance.
(2) every series' record agrees with the CPU oracle under the harmonic tie envelope
    (assert_fit_parity, tests/test_gpu_parity.py, with its own bounds), so that the golden file
    cannot enshrine a wrong parent.

Cases: P = 7 and 133 (ragged series tile, rows beyond P, a second workgroup with 5 live rows);
N = 31, 32, 65, 97, 129, 161 (1 to 6 tiles in one unit: the pipeline's prologue, both halves of
the two-tile loop body, the peeled odd iteration, a partial last tile) and 4099 (17 units of 8
tiles, the last one partial) with 1, 2 and 7 units per workgroup (option upw).  Each for the
ComplexF64 and ComplexF32 storage, all-f64 harmonics (mix = 0), a faint series whose state
changes inside a unit, harmonic fitoffsets (the UNIT instance over the FC columns), a general FC
layout, and FC columns holding a zero and a NaN sample (the phasor fix-up).

The short series span 7.3 modulation periods at a noise of 0.02: that keeps the spread of
NEWUOA's landing points under ulp noise (up to 1.2e-3 with fitoffsets at one period and the
default noise of 0.1) well inside the helper's max_dev of 1e-3.

The tie envelope is a sample.  The oracle re-routes ~15 % of series (~28 % with fitoffsets) under
128-ulp χ² noise, at every length from 31 to 5000 samples, and some of a series' alternative
landing points are rare.  c32/P133/N4099, series 5, is one: the oracle lands on the GPU's point
(b = 2.4097455 against 2.4097262) under 24 of 400 noise seeds, so 12 seeds miss it every other
time.  A series whose GPU record none of the NPERTURB batch runs explains is therefore looked up
under further noise seeds (up to MORE_SEEDS, that series alone); an outcome found there takes
the place of one of the series' draws.  The criterion stays the helper's — the GPU's record is
one the oracle reaches under that noise — and a record the oracle never reaches still fails.

Each case prints its fraction of series within the tolerance.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import synth
from test_gpu_parity import HARM_ULPS, TOL, _dev, assert_fit_parity

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "moments_parent_records.json")
VARIANTS = ("c64", "c32", "mix0", "faint", "offsets", "general", "phasor")
PS = (7, 133)
NS = (31, 32, 65, 97, 129, 161, 4099)
UPWS = (1, 2, 7)
# data seeds: one term per variant, series count and length, all sums distinct
VARIANT_SEED = {"c64": 1000, "c32": 3000, "mix0": 4000, "faint": 5000, "offsets": 7000,
                "general": 8000, "phasor": 6000}
N_SEED = {31: 31, 32: 32, 65: 65, 97: 97, 129: 29, 161: 61, 4099: 25}
NPERTURB = 6  # batch noise runs per case (as smoke() takes); rarer landing points: MORE_SEEDS
MORE_SEEDS = 400  # further noise seeds for a series the batch runs do not explain


def _states(N):
    """NORMAL, then HIGH from the middle on behind a TRANSIENT gap of 3 samples: the change lies
    inside a unit (inside the only tile for N ≤ 32), and both states keep ≥ 12 samples."""
    st = np.full(N, 2, dtype=np.int8)
    st[N // 2:] = 3
    st[N // 2:N // 2 + 3] = -1
    return st


@functools.lru_cache(maxsize=None)
def make_case(variant, P, N):
    """(B, fit keywords, oracle keywords, library options, rows with a NaN FC sample)."""
    seed = VARIANT_SEED[variant] + 10 * P + N_SEED[N]
    short = N < 4099
    B = synth.make_batch(N, P, seed=seed, dt=7.3 / N if short else 0.002,
                         sigma=0.02 if short else 0.1, offsets=variant == "offsets")
    B.pop("truth")
    kw, okw, options = {}, {}, {}
    nan_rows = np.zeros(P, bool)
    if variant == "c32":
        B["d"] = B["d"].astype(np.complex64)
        B["fc"] = B["fc"].astype(np.complex64)
    elif variant == "mix0":
        options["mix"] = 0
    elif variant == "faint":
        st = _states(N)
        B["d"] = B["d"] * np.where(st == 3, 1.1, 0.6)[None, :]
        kw["state"] = okw["state"] = st
    elif variant == "offsets":
        kw["fitoffsets"] = okw["fitoffsets"] = True
    elif variant == "general":
        perm = np.random.default_rng(seed).permutation(P)
        B["d"] = np.ascontiguousarray(B["d"][perm])
        B["fc_of_pixel"] = np.ascontiguousarray(B["fc_of_pixel"][perm])
    elif variant == "phasor":
        G = B["fc"].shape[0]
        B["fc"][0, [3, N - 1]] = 0.0  # angle(0) = 0 → phasor 1, also in the partial last tile
        B["fc"][G - 2, N // 2] = 0.0  # (P = 133: the second workgroup's first group)
        B["fc"][G - 1, N // 2] = complex(np.nan, 0.0)
        nan_rows = B["fc_of_pixel"] == G - 1
    for a in B.values():
        a.setflags(write=False)
    return B, kw, okw, options, nan_rows


@functools.lru_cache(maxsize=None)
def oracle_case(oracle, variant, P, N):
    """run(rows, seed): the oracle's records of the case's series `rows` (None: all) under χ²
    noise of the harmonic evaluator's size (seed 0: none); then the plain and the NPERTURB
    perturbed records of every series — computed once per (variant, P, N), shared by the upw
    cases."""
    B, _, okw, _, _ = make_case(variant, P, N)
    flags = oracle.RECENTER | (oracle.FIT_OFFSETS if okw.get("fitoffsets") else 0)
    d, fc = B["d"].astype(np.complex128), B["fc"].astype(np.complex128)

    def run(rows=None, seed=0):
        rows = np.arange(P) if rows is None else rows
        return oracle.fit_batch(B["t"], d[rows], fc, B["fc_of_pixel"][rows],
                                state=okw.get("state"), flags=flags, perturb_seed=seed,
                                perturb_ulps=HARM_ULPS)
    return run, run(), [run(seed=s) for s in range(1, NPERTURB + 1)]


def _err(x, y):
    return np.max([_dev(x, y, k) for k in ("b", "phi", "a", "chi2")], axis=0)


def deeper_envelope(run, got, ref, pert, rows, tol):
    """For each series of `rows` whose GPU record is within tol of neither the oracle's plain
    record nor one of its perturbed ones: the oracle on that series alone under noise seeds
    1..MORE_SEEDS, until it lands on the GPU's record; that outcome replaces one of the series'
    draws that repeat the plain record.  Returns the perturbed records to hand to the helper."""
    pert = [p.copy() for p in pert]
    seen = (_err(got, ref) <= tol) | np.any([_err(got, p) <= tol for p in pert], axis=0)
    for k in rows[~seen[rows]]:
        dup = [j for j, p in enumerate(pert) if _err(p[k:k + 1], ref[k:k + 1])[0] <= tol]
        for seed in range(1, MORE_SEEDS + 1 if dup else 1):
            o = run(np.array([k]), seed)
            if _err(got[k:k + 1], o)[0] <= tol:
                pert[dup[0]][k] = o[0]
                print(f"series {k}: the oracle reaches the GPU's record under noise seed {seed}")
                break
    return pert


def case_id(variant, P, N, upw):
    return f"{variant}/P{P}/N{N}/upw{upw}"


def fit_case(gpd, variant, P, N, upw):
    B, kw, _, options, _ = make_case(variant, P, N)
    gpd.set_option("upw", upw)
    for k, v in options.items():
        gpd.set_option(k, v)
    return gpd.fit_batch(B["t"], B["d"], B["fc"], B["fc_of_pixel"], method="harmonic", **kw)


def sha(rec):
    return hashlib.sha256(np.ascontiguousarray(rec).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("upw", UPWS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_moment_records(gpu, oracle, opts, variant, P, N, upw):
    opts("upw", upw)  # (registers the reset of every option set by fit_case)
    got = fit_case(gpu, variant, P, N, upw)
    label = case_id(variant, P, N, upw)
    nan_rows = make_case(variant, P, N)[4]
    # (2) against the oracle, every series
    run, ref, pert = oracle_case(oracle, variant, P, N)
    assert np.all(np.isnan(ref["chi2"][nan_rows])) and np.all(np.isnan(got["chi2"][nan_rows]))
    assert np.all(got["status"][nan_rows] & gpu.GPD_ST_NAN)
    assert not np.any(got["status"][~nan_rows] & gpu.GPD_ST_NAN)
    ok = np.nonzero(~nan_rows)[0]
    # (harmonic fitoffsets: the flat offsets landscape, test_offsets_fit_harmonic_on_request)
    offs = variant == "offsets"
    kw = dict(tol=1e-8, min_match=0.5) if offs else dict(tol=TOL, min_match=0.7)
    pert = deeper_envelope(run, got, ref, pert, ok, kw["tol"])
    print(assert_fit_parity(got[ok], ref[ok], [p[ok] for p in pert], label=label, **kw))
    # (1) against the parent build
    assert sha(got) == golden()["records"][label], \
        f"{label}: records differ from the parent build {golden()['build_id']}"


def record(path):
    """Writes the records' hashes of every case, from the library in the tree, to `path`."""
    import gpdemod_loader

    gpd = gpdemod_loader.load()
    rec = {}
    for variant in VARIANTS:
        for P in PS:
            for N in NS:
                for upw in UPWS:
                    rec[case_id(variant, P, N, upw)] = sha(fit_case(gpd, variant, P, N, upw))
                    gpd.reset_options()
    with open(path, "w") as fh:
        json.dump({"build_id": gpd.build_id(), "records": rec}, fh, indent=0, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    import sys

    import torch  # noqa: F401  (before the library, as in conftest.py)

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1])
