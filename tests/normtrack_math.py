"""numpy fp64 restatement of dvq_segment_stats (docs/design/24-norm-tracking.md) and of the host-side grouping of normtrack.py: what
the kernels and the aggregation must compute, written without reference to how they compute it."""
import numpy as np


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def segment_stats(a, offsets, b=None):
    """per segment: fp64 sum of the exact squares of the finite elements, fp32 abs-max of the finite elements, count of the others;
    with b the element is a - b in fp64 (exact for fp32 operands), non-finite where either operand is"""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    fin = np.isfinite(a64)
    if b is not None:
        b64 = np.asarray(b, dtype=np.float32).astype(np.float64)
        fin &= np.isfinite(b64)
        with np.errstate(invalid="ignore"):
            a64 = a64 - b64
    v = np.where(fin, a64, 0.0)
    S = len(offsets) - 1
    sumsq, absmax, bad = np.zeros(S, np.float64), np.zeros(S, np.float32), np.zeros(S, np.int64)
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        sumsq[s] = np.sum(v[lo:hi] * v[lo:hi])
        with np.errstate(over="ignore"):
            absmax[s] = np.float32(np.max(np.abs(v[lo:hi])))
        bad[s] = int((~fin[lo:hi]).sum())
    return sumsq, absmax, bad


def sticky(bad_per_launch):
    """running totals and first offending launch (0-based, -1: none) per segment over a list of per-launch counts"""
    bad = np.asarray(bad_per_launch, dtype=np.int64)
    total = bad.sum(axis=0)
    first = np.full(bad.shape[1], -1, np.int64)
    for s in range(bad.shape[1]):
        hit = np.nonzero(bad[:, s])[0]
        if hit.size:
            first[s] = hit[0]
    return total, first


def group(stats, depth):
    """{prefix of `depth` dotted components: aggregated entry} of a {name: entry} dict: squares add, abs-max takes the max, counts add"""
    out = {}
    for name, e in stats.items():
        key = name if depth <= 0 else ".".join(name.split(".")[:depth])
        g = out.setdefault(key, {"numel": 0, "g2": 0.0, "w2": 0.0, "u2": 0.0, "absmax": 0.0, "bad": 0})
        g["numel"] += e["numel"]
        g["g2"] += float(e["grad_norm"]) ** 2
        g["w2"] += float(e["weight_norm"]) ** 2
        g["u2"] += float(e["update_norm"]) ** 2
        g["absmax"] = max(g["absmax"], float(e["grad_absmax"]))
        g["bad"] += e["grad_nonfinite"]
    return out
