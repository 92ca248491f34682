"""Fixtures for the segment metrics (tests/golden/metrics/*.npz): scores and labels, and what sklearn.metrics
returns for them, so that the GPU tests need no sklearn.  Data only.

Each file holds: scores [n] float32, labels [n] float32, thresholds [T] float32, sklearn's accuracy, precision
and recall of `scores > t` per threshold (float64 [T]), its full roc_curve (drop_intermediate=False: roc_fpr,
roc_tpr, roc_thresholds) and roc_auc_score.  The files are written with fixed zip timestamps, so a rerun
reproduces them bit for bit.

usage: python tools/gen_metrics_golden.py
"""
import io
import os
import zipfile

import numpy as np
from sklearn.metrics import accuracy_score, precision_score, recall_score, roc_auc_score, roc_curve

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "metrics")
THRESHOLDS = np.array([0.5, 0.25, 0.75, 0.1, 0.9, 0.0, np.float32(0.5) + np.float32(2 ** -24)], dtype=np.float32)


def adversarial(seed, n=6000):
    """Uniform scores with exact thresholds, exact bin edges (at 1 .. 8192 bins per octave), 0, 1, subnormals,
    ties; labels correlated with the scores."""
    rng = np.random.default_rng(seed)
    e = rng.random(n, dtype=np.float32)
    special = np.concatenate([
        THRESHOLDS, np.float32([0.0, 1.0, 1e-45, 1e-40, 2 ** -126, 2 ** -30, 0.5, 0.5, 0.5]),
        (rng.integers(0x30000000, 0x3F800000, 200).astype(np.uint32) & np.uint32(0xFFFFFC00)).view(np.float32),  # edges
        np.nextafter(np.float32(0.5), np.float32(0), dtype=np.float32) * np.ones(5, np.float32)])
    e[:special.size] = special
    e[special.size:special.size + 500] = e[special.size]                     # a pile of ties
    rng.shuffle(e)
    y = (rng.random(n) < 0.2 + 0.6 * e).astype(np.float32)
    return e, y


def clustered(seed, n=8000):
    """sigmoid of normals: fakes near 0 over many octaves, trues piled up near 1 (a trained model's shape)."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.3).astype(np.float32)
    x = np.where(y == 1, rng.normal(6, 3, n), rng.normal(-7, 3, n))
    return (1 / (1 + np.exp(-x))).astype(np.float32), y


def from_fixture(name, seed):
    """A fixture's recorded forward scores, with seeded labels that lean on the score."""
    e = np.load(os.path.join(REPO, "tests", "golden", name + ".npz"))["scores"].astype(np.float32).reshape(-1)
    rng = np.random.default_rng(seed)
    return e, (rng.random(e.size) < e).astype(np.float32)


def record(e, y):
    fpr, tpr, thr = roc_curve(y, e, drop_intermediate=False)
    return {"scores": e, "labels": y, "thresholds": THRESHOLDS,
            "accuracy": np.array([accuracy_score(y, e > t) for t in THRESHOLDS]),
            "precision": np.array([precision_score(y, e > t, zero_division=0.0) for t in THRESHOLDS]),
            "recall": np.array([recall_score(y, e > t, zero_division=0.0) for t in THRESHOLDS]),
            "roc_fpr": fpr, "roc_tpr": tpr, "roc_thresholds": thr.astype(np.float64),
            "roc_auc": np.float64(roc_auc_score(y, e))}


def save(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(path, os.path.getsize(path), "bytes")


def main():
    os.makedirs(OUT, exist_ok=True)
    save("adversarial_s0", record(*adversarial(0)))
    save("clustered_s1", record(*clustered(1)))
    save("fixture_c2_scale", record(*from_fixture("c2_scale_s0", 2)))
    save("fixture_sector_d64", record(*from_fixture("sector_d64_s0", 3)))


if __name__ == "__main__":
    main()
