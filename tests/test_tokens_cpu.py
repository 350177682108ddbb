"""Host half of the token shards (docs/design/16-token-shards.md): record format, writer / dataset round trips, refused sets,
check_model, the host-side row lengths against oracle/permuter.py, the loader's index / view plan.  No GPU, no library."""
import json
import os
import types

import numpy as np
import pytest

from dynamicvectorquantization_amd import tokens as T
from oracle import permuter as OP

HW1, HW2, KCODES = 4, 2, 512


def make_records(n, views=1, seed=0, hw1=HW1, hw2=HW2, k=KCODES):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=T.record_dtype(hw1, hw2))
    grain = (rng.random((n, hw1, hw1)) < 0.5).astype(np.int64)
    rec["codes"] = rng.integers(0, k, size=(n, hw1 * hw2, hw1 * hw2))
    rec["codes"][0, 0, 0] = k - 1
    rec["grain"] = T.pack_grain_bits(grain)
    rec["n_fine_cells"] = grain.reshape(n, -1).sum(1)
    rec["label"] = rng.integers(0, 10, size=n)
    rec["source"] = np.arange(n) // views
    rec["view"] = np.arange(n) % views
    return rec, grain


def write_set(path, rec, views=("center",), shard_size=5, part=None, fingerprint="f" * 64, **kw):
    w = T.TokenShardWriter(path, HW1, HW2, KCODES, list(views), shard_size=shard_size, compute_dtype="fp32", fingerprint=fingerprint,
                           dataset={"synthetic": 12}, part=part, **kw)
    w.append_records(rec[:3])          # batches that do not line up with the file roll
    w.append_records(rec[3:])
    return w.close()


def test_record_layout():
    dt = T.record_dtype(16, 2)
    assert dt.itemsize == 32 * 32 * 2 + 8 * 4 + 2 + 4 + 4 + 1 == 2091            # ~2.1 KB per ImageNet view
    assert dt["codes"].shape == (32, 32) and dt["grain"].shape == (8,)
    g = np.zeros((1, 12, 12), dtype=np.int64)
    g[0, 0, 0] = g[0, 2, 8] = g[0, 11, 11] = 1                                    # cells 0, 32, 143
    bits = T.pack_grain_bits(g)
    assert bits.dtype == np.dtype("<u4") and bits.shape == (1, 5)
    assert bits[0].tolist() == [1, 1, 0, 0, 1 << (143 % 32)]
    assert np.array_equal(T.unpack_grain_bits(bits, 12), g) and T.popcount_rows(bits).tolist() == [3]
    g[0, 5, 5] = 2                                                                # not a grain: stored as coarse
    assert np.array_equal(T.pack_grain_bits(g), bits)


def test_round_trip_across_a_file_roll(tmp_path):
    rec, _ = make_records(12)
    meta = write_set(tmp_path / "set", rec, shard_size=5)
    assert [f["records"] for f in meta["files"]] == [5, 5, 2]
    assert sorted(os.listdir(tmp_path / "set")) == ["meta.json", "tokens-00000.npy", "tokens-00001.npy", "tokens-00002.npy"]
    one = np.load(tmp_path / "set" / "tokens-00001.npy", mmap_mode="r")              # a plain .npy: random access through numpy alone
    assert one.dtype == rec.dtype and one[2].tobytes() == rec[7].tobytes()
    ds = T.TokenShardDataset(tmp_path / "set", verify=True)
    assert len(ds) == 12 and ds.n_records == 12 and ds.n_views == 1
    assert ds.records(np.arange(12)).tobytes() == rec.tobytes()
    pick = np.array([11, 0, 5, 4, 7, 7])
    assert ds.records(pick).tobytes() == rec[pick].tobytes()
    for k in ("version", "hw1", "hw2", "codebook_size", "views", "n_views", "files", "compute_dtype", "fingerprint", "dataset"):
        assert k in ds.meta, k
    with pytest.raises(IndexError):
        ds.records([12])


def test_round_trip_across_two_parts(tmp_path):
    rec, _ = make_records(12, views=2)
    out = tmp_path / "set"
    write_set(out, rec[8:], views=("center", "flip"), shard_size=3, part=(1, 2))
    with pytest.raises(T.TokenSetError, match="meta.json"):
        T.TokenShardDataset(out)                                                  # parts without --finalize: incomplete
    with pytest.raises(T.TokenSetError, match="parts"):
        T.finalize_parts(out)                                                     # part 0 is missing
    write_set(out, rec[:8], views=("center", "flip"), shard_size=3, part=(0, 2))
    meta = T.finalize_parts(out)
    assert [f["name"] for f in meta["files"]] == ["tokens-p0000-00000.npy", "tokens-p0000-00001.npy", "tokens-p0000-00002.npy",
                                                  "tokens-p0001-00000.npy", "tokens-p0001-00001.npy"]
    ds = T.TokenShardDataset(out, verify=True)
    assert len(ds) == 6 and ds.n_records == 12
    assert ds.records(np.arange(12)).tobytes() == rec.tobytes()
    assert ds.gather([5, 0], [1, 0]).tobytes() == rec[[11, 0]].tobytes()


def test_inconsistent_parts_are_refused(tmp_path):
    rec, _ = make_records(4)
    write_set(tmp_path / "s", rec[:2], part=(0, 2))
    write_set(tmp_path / "s", rec[2:], part=(1, 2), fingerprint="e" * 64)
    with pytest.raises(T.TokenSetError, match="fingerprint"):
        T.finalize_parts(tmp_path / "s")


def test_refused_sets(tmp_path):
    rec, _ = make_records(12)

    def fresh(name, r=rec):
        write_set(tmp_path / name, r)
        return tmp_path / name

    p = fresh("no_meta")
    os.remove(p / "meta.json")
    with pytest.raises(T.TokenSetError, match="incomplete"):
        T.TokenShardDataset(p)

    p = fresh("version")
    meta = json.loads((p / "meta.json").read_text())
    meta["version"] = 99
    (p / "meta.json").write_text(json.dumps(meta))
    with pytest.raises(T.TokenSetError, match="version"):
        T.TokenShardDataset(p)

    p = fresh("truncated")
    size = os.path.getsize(p / "tokens-00001.npy")
    with open(p / "tokens-00001.npy", "r+b") as f:
        f.truncate(size - 7)
    with pytest.raises(T.TokenSetError, match="tokens-00001"):
        T.TokenShardDataset(p)

    bad = rec.copy()
    bad["codes"][9, 1, 1] = KCODES                       # last record of the second file: found at open time
    with pytest.raises(T.TokenSetError, match="codebook_size"):
        T.TokenShardDataset(fresh("code_edge", bad))
    bad = rec.copy()
    bad["codes"][7, 1, 1] = KCODES                       # in the middle of a file: found by the full check
    p = fresh("code_middle", bad)
    T.TokenShardDataset(p)
    with pytest.raises(T.TokenSetError, match="codebook_size"):
        T.TokenShardDataset(p, verify=True)

    bad = rec.copy()
    bad["n_fine_cells"][0] += 1
    with pytest.raises(T.TokenSetError, match="n_fine_cells"):
        T.TokenShardDataset(fresh("count_edge", bad))
    bad = rec.copy()
    bad["n_fine_cells"][7] += 1
    p = fresh("count_middle", bad)
    with pytest.raises(T.TokenSetError, match="n_fine_cells"):
        T.TokenShardDataset(p, verify=True)
    ds = T.TokenShardDataset(p)                          # the loader's own check catches it when the record is read
    r = ds.records([6, 7])
    with pytest.raises(T.TokenSetError, match="n_fine_cells"):
        T.batch_lengths(r["grain"], r["n_fine_cells"], HW1, HW2)


def fake_model(hw1=HW1, hw2=HW2, k=KCODES, weight_seed=0, threshold=1.5):
    import torch
    w = torch.from_numpy(np.random.default_rng(weight_seed).standard_normal((k, 8)).astype(np.float32))
    router = types.SimpleNamespace(fine_grain_threshold=threshold) if threshold is not None else types.SimpleNamespace()
    fs = types.SimpleNamespace(quantize=types.SimpleNamespace(codebook=types.SimpleNamespace(weight=w, n_embed=k)),
                               encoder=types.SimpleNamespace(router=router))
    return types.SimpleNamespace(hw1=hw1, hw2=hw2, first_stage_model=fs)


def test_check_model(tmp_path):
    rec, _ = make_records(4)
    model = fake_model()
    fp = T.first_stage_fingerprint(model.first_stage_model)
    assert len(fp) == 64 and fp == T.first_stage_fingerprint(fake_model().first_stage_model)
    write_set(tmp_path / "s", rec, fingerprint=fp)
    ds = T.TokenShardDataset(tmp_path / "s")
    ds.check_model(model)
    with pytest.raises(T.TokenSetError, match="hw1"):
        ds.check_model(fake_model(hw1=8))
    for other in (fake_model(weight_seed=1), fake_model(threshold=1.25)):
        ofp = T.first_stage_fingerprint(other.first_stage_model)
        assert ofp != fp
        with pytest.raises(T.TokenSetError) as e:
            ds.check_model(other)
        assert fp in str(e.value) and ofp in str(e.value)
    assert T.first_stage_fingerprint(fake_model(threshold=None).first_stage_model) == "feature-router"


@pytest.mark.parametrize("hw1,hw2", [(4, 2), (12, 2), (8, 4)])
@pytest.mark.parametrize("order", ["region-first", "row-first"])
def test_host_side_lengths_match_the_oracle(hw1, hw2, order):
    rng = np.random.default_rng(hw1 * 10 + hw2)
    fhw = hw1 * hw2
    cases = {"all coarse": np.zeros((3, hw1, hw1), dtype=np.int64), "all fine": np.ones((3, hw1, hw1), dtype=np.int64),
             "mixed": (rng.random((5, hw1, hw1)) < 0.4).astype(np.int64)}
    cases["mixed"][0] = 0
    cases["one of each"] = np.stack([np.zeros((hw1, hw1), dtype=np.int64), np.ones((hw1, hw1), dtype=np.int64)])
    for name, grain in cases.items():
        idx = rng.integers(0, 1024, size=(grain.shape[0], fhw, fhw))
        want = OP.forward(idx, grain, hw1, hw2, order)
        bits = T.pack_grain_bits(grain)
        n, lc, lf = T.batch_lengths(bits, grain.reshape(grain.shape[0], -1).sum(1), hw1, hw2)
        assert (lc, lf) == (want["coarse_content"].shape[1], want["fine_content"].shape[1]), name
        assert n.tolist() == grain.reshape(grain.shape[0], -1).sum(1).tolist()


def test_view_plan_is_reproducible_and_uses_both_views():
    def plan(seed, **kw):
        return T.plan_epoch(10, 2, 4, True, True, np.random.default_rng(seed), **kw)
    a, b, c = plan(3), plan(3), plan(4)
    assert len(a) == 2 and all(len(i) == 4 and len(v) == 4 for i, v in a)                  # drop_last: 10 // 4
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert not all(np.array_equal(x[0], y[0]) for x, y in zip(a, c))
    images = np.concatenate([i for i, _ in a])
    assert len(set(images.tolist())) == 8 and images.min() >= 0 and images.max() < 10
    assert set(np.concatenate([v for _, v in a]).tolist()) == {0, 1}
    full = T.plan_epoch(10, 2, 4, False, False, np.random.default_rng(0), view=1)           # evaluation: stored order, a fixed view
    assert np.array_equal(np.concatenate([i for i, _ in full]), np.arange(10)) and len(full) == 3
    assert set(np.concatenate([v for _, v in full]).tolist()) == {1}
    with pytest.raises(ValueError):
        T.plan_epoch(10, 2, 4, False, False, np.random.default_rng(0), view=2)


def test_module_imports_without_the_library():
    import subprocess
    import sys
    code = ("import sys; import dynamicvectorquantization_amd.tokens as T; "
            "assert 'dynamicvectorquantization_amd._lib' not in sys.modules and 'torch' not in sys.modules; print(T.FORMAT_VERSION)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and r.stdout.strip() == "1", r.stderr[-2000:]
