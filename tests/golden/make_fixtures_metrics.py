#!/usr/bin/env python
"""Writes tests/golden/metrics.npz: the reference's own values of the evaluation metrics (scripts/Clustering.py) on the seeded
inputs of tests/_metrics_inputs.py.  Seeds, shapes, sha256 of the inputs and the expected scalars only -- no large arrays.

    python tests/golden/make_fixtures_metrics.py --reference <checkout of the reference>/scripts

The reference's `Clustering` module is imported unchanged, with stub modules for what the image lacks.  Exercised:
  * calculate_frechet_distance (:1252-1315), fed np.mean(axis=0) / np.cov(rowvar=False) exactly as frechet_distance (:1376-1385) does;
    the run is checked to stay on the real, finite path (no complex sqrtm output, no eps fallback);
  * hellinger (:1635-1646);
  * the two expressions at :1394 (scipy.stats.wasserstein_distance over range(K)) and :1540 (perplexity)."""
import argparse
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _metrics_inputs as MI  # noqa: E402


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(self.__name__ + "." + name)

    def __call__(self, *a, **k):
        return None


def import_clustering(ref_scripts: str):
    for name in ("seaborn", "openTSNE", "transforms3d", "librosa", "librosa.display", "lmdb", "torchvision", "torchvision.utils",
                 "fasttext", "config", "config.parse_args", "pyarrow", "soundfile"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Stub(name)
    try:
        importlib.import_module("configargparse")
    except Exception:
        m = _Stub("configargparse")
        m.argparse = argparse
        sys.modules["configargparse"] = m
    sys.path.insert(0, ref_scripts)
    return importlib.import_module("Clustering")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's scripts/ directory")
    ap.add_argument("--out", default=os.path.join(HERE, "metrics.npz"))
    a = ap.parse_args()
    C = import_clustering(os.path.abspath(a.reference))
    from scipy import linalg, stats
    out = {}
    for case, (n1, n2, E) in MI.FRECHET_CASES.items():
        A, B = MI.frechet_inputs(case)
        mu1, s1, mu2, s2 = np.mean(A, axis=0), np.cov(A, rowvar=False), np.mean(B, axis=0), np.cov(B, rowvar=False)
        root, _ = linalg.sqrtm(s1.dot(s2), disp=False)
        assert np.isfinite(root).all() and (not np.iscomplexobj(root) or np.abs(root.imag).max() == 0.0), \
            f"{case}: the reference leaves its real, finite path here"
        with contextlib.redirect_stdout(io.StringIO()):
            fd = float(C.calculate_frechet_distance(mu1, s1, mu2, s2))
        out[f"frechet/{case}/shape"] = np.array([n1, n2, E], dtype=np.int64)
        out[f"frechet/{case}/sha256"] = np.array([MI.sha256(A), MI.sha256(B)])
        out[f"frechet/{case}/value"] = np.float64(fd)
        print(f"frechet {case}: {fd:.10g}")
    for case in MI.HIST_CASES:
        i1, i2 = MI.hist_inputs(case)
        h1 = np.bincount(i1, minlength=MI.HIST_K).astype(np.float64)
        h2 = np.bincount(i2, minlength=MI.HIST_K).astype(np.float64)
        assert (h1 == 0).any() and (h2 == 0).any()
        p, q = h1 / np.sum(h1), h2 / np.sum(h2)
        dists = [i for i in range(len(p))]
        out[f"hist/{case}/sha256"] = np.array([MI.sha256(i1), MI.sha256(i2)])
        out[f"hist/{case}/hellinger"] = np.float64(C.hellinger(h1, h2))
        out[f"hist/{case}/wasserstein"] = np.float64(stats.wasserstein_distance(dists, dists, p, q))
        out[f"hist/{case}/perplexity"] = np.array([np.exp(-np.sum(p * np.log(p + +1e-10))), np.exp(-np.sum(q * np.log(q + +1e-10)))])
        print(f"hist {case}:", out[f"hist/{case}/hellinger"], out[f"hist/{case}/wasserstein"], out[f"hist/{case}/perplexity"])
    np.savez(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
