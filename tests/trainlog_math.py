"""fp64 numpy restatement of the two training-log kernels (include/dvq_hip.h: dvq_scalar_push, dvq_codebook_health).  No GPU, no library:
the GPU tests compare the kernels to this, the CPU tests check it against hand-worked cases."""
import numpy as np

F32, BF16, F64, I32, I64, IMM, SKIP = range(7)


def new_state(columns):
    return {"sum": np.zeros(columns, np.float64), "cnt": np.zeros(columns, np.int64), "bad": np.zeros(columns, np.int64),
            "last": np.zeros(columns, np.float32)}


def bf16_round(x):
    """nearest-even bf16 of fp32 values, as fp32 (NaN / Inf pass through)"""
    x = np.asarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(x), r, x).astype(np.float32)


def typed(code, v):
    """the value as the element type of `code` holds it (what the device tensor contains)"""
    if code == F32:
        return np.float32(v)
    if code == BF16:
        return np.float32(bf16_round(np.float32(v)))
    if code in (F64, IMM):
        return np.float64(v)
    if code == I32:
        return np.int32(v)
    return np.int64(v)


def scalar_push(state, codes, values, col0=0):
    """one push: column col0 + i gets values[i] (already `typed`), in place; SKIP leaves the column alone"""
    with np.errstate(over="ignore", invalid="ignore"):
        for i, (code, v) in enumerate(zip(codes, values)):
            if code == SKIP:
                continue
            c = col0 + i
            v64 = np.float64(v)
            state["last"][c] = np.float32(v)
            if np.isfinite(v64):
                state["sum"][c] = state["sum"][c] + v64
                state["cnt"][c] += 1
            else:
                state["bad"][c] += 1
    return state


def codebook_health(counts):
    """counts [K] -> (perplexity, active codes, tokens) in fp64; all-zero counts: (0, 0, 0)"""
    n = np.asarray(counts, np.float64)
    s = float(n.sum())
    if not s > 0.0:
        return 0.0, 0.0, s
    p = n[n > 0] / s
    return float(np.exp(-(p * np.log(p)).sum())), float((n > 0).sum()), s
