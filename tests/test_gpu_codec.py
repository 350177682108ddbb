"""The lossless token codec on the GPU (docs/design/27-token-codec.md).  Kernel level: dvq_codec_tables / _record / _encode /
_decode_step against the op-by-op mask functions of the sampler, an fp64 softmax and the numpy restatement (tests/codec_math.py).
Model level: Dualformer.compress / decompress of the small unconditional and class-conditional models, exact round trips."""
import zlib

import numpy as np
import pytest
import torch

import codec_math as cm

pytestmark = pytest.mark.gpu

M = cm.M
KINDS = ("coarse_pos", "fine_pos", "content", "free")


def _kinds(v):
    """the content rule forbids three special codes: below four columns it leaves a live row nothing to code"""
    return [k for k in KINDS if v >= 4 or k != "content"]


# ---------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------
def _rules_model(v):
    """a bare sampler mixin whose codes sit at the top of a V-column vocabulary: cells / codes 0 .. V-4, <pad> V-3, <eos> V-2, <sos>
    V-1 (V = 2: <pad> 0, <eos> 1 and no <sos> column).  max_coarse_postion_idx is LIFTED to the pad code: the codec's one change"""
    from dynamicvectorquantization_amd.stage2 import _SamplerMixinBase
    df = _SamplerMixinBase.__new__(_SamplerMixinBase)
    pad, eos, sos = (v - 3, v - 2, v - 1) if v >= 3 else (0, 1, 0)
    df.__dict__.update(coarse_position_pad_code=pad, coarse_position_eos_code=eos, max_coarse_postion_idx=pad, fine_position_pad_code=pad,
                       fine_position_eos_code=eos, fine_position_sos_code=sos, content_pad_code=pad, content_eos_code=eos,
                       content_sos_code=sos)
    return df


def _rule_kw(df, kind):
    from dynamicvectorquantization_amd import codec
    if kind == "free":                                   # no constraint at all: n = V on a live row
        return dict(pad_code=df.content_pad_code)
    return codec.codec_rule(df, kind)


def _op_by_op(df, kind, logits, sampled, done):
    """the sampler's mask functions on fp32 logits -> bool [B, V]: the columns left finite"""
    from dynamicvectorquantization_amd.stage2 import _mask_rows
    lg = logits.float().clone()
    if kind == "coarse_pos":
        out = df.avoid_repeat_or_enforce_pad_for_coarse_position(lg, sampled, done)
    elif kind == "fine_pos":
        out = df.avoid_repeat_or_enforce_pad_for_fine_position(lg, sampled, done)
    elif kind == "content":
        out = df.avoid_special_or_enforce_pad_for_content(lg, done)
    else:
        out = _mask_rows(lg, done, torch.zeros_like(lg, dtype=torch.bool), None, df.content_pad_code)
    return torch.isfinite(out)


def _case(dev, b, v, dtype, strided, kind, seed):
    """logits [B, V] (a column slice of a wider matrix when strided), the forbid lists, done flags; with B >= 5 the LAST row is left
    with a single allowed symbol and row 1 is finished (B = 1: one ordinary live row)"""
    g = torch.Generator().manual_seed(seed)
    wide = v + 5 if strided else v
    base = (3.0 * torch.randn(b, wide, generator=g)).to(dtype).to(dev)       # |x - max| stays far from fp32 exp underflow
    logits = base[:, :v]
    df = _rules_model(v)
    cells = max(v - 3, 1)
    sampled = torch.randint(0, cells, (b, max(cells, 2)), generator=g)
    sampled[:, cells // 3:] = sampled[:, :1]                                 # about a third of the cells drawn already
    done = torch.zeros(b, 1)
    if b >= 5:
        done[1] = 1
    single = b - 1
    if b < 5:
        pass
    elif kind in ("coarse_pos", "fine_pos"):
        sampled[single, :cells] = torch.arange(cells)                        # every cell drawn: only <eos> is left
    else:
        keep = int(torch.randint(0, cells, (1,), generator=g))
        row = torch.full((wide,), float("-inf"))
        row[keep] = 0.25
        base[single] = row.to(dtype).to(dev)                                 # -inf logits leave the allowed set
    return df, logits, sampled.to(dev), done.to(dev)


def _tables(logits, df, kind, sampled, done):
    from dynamicvectorquantization_amd import kernels as K
    kw = _rule_kw(df, kind)
    if kind in ("coarse_pos", "fine_pos"):
        kw["forbid_idx"] = sampled
    return K.codec_tables(logits, finished=done, **kw), kw


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("v", [2, 63, 64, 65, 259, 1027, 2048])
def test_tables_invariants_masks_accuracy(dev, v, dtype):
    """for B in {1, 5, 16}, dense and strided logits and every rule: sum f = M, f >= 1 exactly on the op-by-op allowed set, f = 0
    elsewhere; a finished row and a single-symbol row put M on their one column; every non-arg-max allowed column has
    |f - 1 - p (M - n)| <= 1 + eps M p against an fp64 softmax, eps = 4 x the worst relative deviation of torch's fp32 softmax from
    fp64 on the same rows (floor 2^-20)"""
    worst, worst_eps = -1.0, 0.0
    for b in (1, 5, 16):
        for strided in (False, True):
            for ki, kind in enumerate(_kinds(v)):
                df, logits, sampled, done = _case(dev, b, v, dtype, strided, kind, seed=v * 131 + b * 7 + ki)
                f, _ = _tables(logits, df, kind, sampled, done)
                f = f.long()
                allowed = _op_by_op(df, kind, logits, sampled, done)
                assert torch.equal(f.sum(dim=1), torch.full((b,), M, device=dev)), (b, strided, kind)
                assert torch.equal(f > 0, allowed), (b, strided, kind)
                n = allowed.sum(dim=1)
                if b >= 5:
                    assert int(n[b - 1]) == 1 and int(f[b - 1].max()) == M              # the single-symbol row
                    assert int(f[1, df.content_pad_code]) == M                          # the finished row
                x64 = logits.double().masked_fill(~allowed, float("-inf"))
                p64 = torch.softmax(x64, dim=1)
                p32 = torch.softmax(logits.float().masked_fill(~allowed, float("-inf")), dim=1).double()
                rel = ((p32 - p64).abs() / p64.clamp_min(1e-300))[allowed]
                eps = max(4.0 * float(rel.max()), 2.0 ** -20)
                tie = allowed & (x64 == x64.max(dim=1, keepdim=True)[0])
                amax = tie & (torch.cumsum(tie.long(), dim=1) == 1)                     # the LOWEST arg-max takes the remainder
                check = allowed & ~amax & (n > 1).view(-1, 1)
                dev_abs = (f.double() - 1.0 - p64 * (M - n).double().view(-1, 1)).abs()
                slack = dev_abs - (1.0 + eps * M * p64)
                assert not bool((slack[check] > 0).any()), (b, strided, kind, float(slack[check].max()))
                if bool(check.any()):                                                   # what the bound's eps term has to cover
                    worst = max(worst, float(((dev_abs - 1.0) / (M * p64))[check].max()))
                    worst_eps = max(worst_eps, eps)
    print(f"codec_tables V={v} {dtype}: worst (|f - 1 - p (M - n)| - 1) / (M p) = {worst:.3e}; eps up to {worst_eps:.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("v", [2, 63, 64, 65, 259, 1027, 2048])
def test_record_and_decode_step_match_table(dev, v, dtype):
    """for B in {1, 5, 16}, dense and strided logits and every rule: dvq_codec_record's (cum, f) are the table's at the target, a
    forbidden or out-of-range target sets that row's error word and codes nothing; the one-symbol stream dvq_codec_encode makes of the
    record decodes through dvq_codec_decode_step to the same token, state L and cursor at the word count"""
    for b in (1, 5, 16):
        for strided in (False, True):
            for ki, kind in enumerate(_kinds(v)):
                _record_decode_case(dev, b, v, dtype, strided, kind, seed=v * 17 + b * 5 + ki)


def _record_decode_case(dev, b, v, dtype, strided, kind, seed):
    from dynamicvectorquantization_amd import kernels as K
    df, logits, sampled, done = _case(dev, b, v, dtype, strided, kind, seed=seed)
    f, kw = _tables(logits, df, kind, sampled, done)
    f = f.long()
    cum = torch.cumsum(f, dim=1) - f
    target = torch.multinomial((f > 0).float(), 1).view(-1)                      # an allowed symbol per row
    records = torch.full((b, 4), -1, dtype=torch.int32, device=dev)
    err = torch.zeros(b, dtype=torch.int32, device=dev)
    tok = K.codec_record(logits, target, records, 2, err, finished=done, **kw)
    n = (f > 0).sum(dim=1)
    live = (done.view(-1) == 0) & (n > 1)
    ft, ct = f.gather(1, target.view(-1, 1)).view(-1), cum.gather(1, target.view(-1, 1)).view(-1)
    want = torch.where(live, ct | (ft << 16), torch.zeros_like(ct))
    assert torch.equal(records[:, 2].long() & 0xFFFFFFFF, want), kind
    assert bool((records[:, [0, 1, 3]] == -1).all())                            # only column `step` is written
    assert int(err.abs().sum()) == 0
    want_tok = torch.where(done.view(-1) != 0, torch.full_like(target, kw["pad_code"]), target)
    assert torch.equal(tok.view(-1), want_tok)
    # the one-step stream of every row, decoded: the search finds the target's column whichever lane owns it
    words, nwords, _ = K.codec_encode(records[:, 2:3].contiguous(), 1)
    flat = words.reshape(-1).contiguous()
    state = K.codec_decode_state(flat, torch.arange(b, device=dev) * 3 + 3 - nwords, nwords)
    err2 = torch.zeros(b, dtype=torch.int32, device=dev)
    got = K.codec_decode_step(logits, state, flat, err2, finished=done, **kw)
    assert torch.equal(got, tok), (kind, b, strided)
    assert int(err2.abs().sum()) == 0 and bool((state[:, 0] == cm.L).all()) and torch.equal(state[:, 1], nwords)
    # a forbidden target on row 0 (live): the error word of that row only, and a record that codes nothing
    bad_cols = torch.nonzero(f[0] == 0).view(-1)
    if bad_cols.numel():
        target2 = target.clone()
        target2[0] = bad_cols[0]
        records.fill_(-1)
        K.codec_record(logits, target2, records, 0, err, finished=done, **kw)
        assert int(err[0]) & 1 and int(err[1:].abs().sum()) == 0, (kind, b)
        assert int(records[0, 0]) == 0
    err.zero_()
    target3 = target.clone()
    target3[0] = v + 3                                                           # outside the vocabulary
    K.codec_record(logits, target3, records, 1, err, finished=done, **kw)
    assert int(err[0]) & 1 and int(records[0, 1]) == 0


@pytest.mark.parametrize("v", [2, 63, 64, 65, 259, 1027, 2048])
def test_tables_against_restatement(dev, v):
    """dvq_codec_tables against tests/codec_math.table on fp32 logits.  Rows whose exponentials are exactly 0 or 1 in any libm (ties at
    the maximum over -inf and -200 columns) must agree BIT FOR BIT: that pins the allowed set, n, the fp32 quotient and product, the floor and
    the remainder's column (S is a small integer there, exact in any order).  On random rows numpy's exp and the device's expf may differ in the last place, which
    moves a floor by at most one: every column within 1, the remainder column within the number of columns that moved"""
    from dynamicvectorquantization_amd import kernels as K
    g = torch.Generator().manual_seed(900 + v)
    rows = []
    for frac in (1.0, 0.5, 0.1):                                   # a fraction of the columns tied at the maximum, the rest far below
        x = torch.full((v,), -200.0)
        tied = torch.rand(v, generator=g) < frac
        tied[0] = tied[v - 1] = True
        x[tied] = 1.5
        x[torch.rand(v, generator=g) < 0.1] = float("-inf")
        x[v - 1] = 1.5
        rows.append(x)
    exact = len(rows)
    rows += [s_ * torch.randn(v, generator=g) for s_ in (0.5, 3.0, 10.0)]
    logits = torch.stack(rows)
    f = K.codec_tables(logits.to(dev), pad_code=0).cpu().numpy().astype(np.int64)
    for r, x in enumerate(logits.numpy()):
        ref = cm.table(x, cm.allowed_mask(x)).astype(np.int64)
        if r < exact:
            assert np.array_equal(f[r], ref), (v, r)
        else:
            amax = int(np.argmax(x))
            diff = np.abs(f[r] - ref)
            moved = int((np.delete(diff, amax) != 0).sum())
            assert int(np.delete(diff, amax).max(initial=0)) <= 1 and int(diff[amax]) <= moved, (v, r, moved)
            assert int(f[r].sum()) == M and np.array_equal(f[r] > 0, ref > 0)


def test_sampler_and_codec_share_one_rule(dev):
    """the same rule keywords through both kernels, at the codec's lane-stride edges and the sampler's sort-size steps (256 / 512 / 1024
    threads), fp32 and bf16, B in {1, 5}, dense and strided logits, every rule kind:
    (a) the greedy draw (temperature 1, no top-k / top-p) is, per row, the lowest-index arg-max of the logits over the columns the
        codec gives a frequency to -- pad_code on the finished row, the one column of the single-symbol row;
    (b) dvq_sample_guided at guidance 1 on [logits ; other random logits] with the 2B-row lists and flags returns those tokens in both
        halves.
    And a bad rule (pad_code = V, pad_code < 0) or V = 2049 is refused by all five wrappers with a DvqError, nothing written."""
    from dynamicvectorquantization_amd import kernels as K
    for v in (2, 64, 65, 256, 257, 1024, 1025, 2048):
        for di, dtype in enumerate((torch.float32, torch.bfloat16)):
            for b in (1, 5):
                for strided in (False, True):
                    for ki, kind in enumerate(_kinds(v)):
                        what = (v, dtype, b, strided, kind)
                        df, logits, sampled, done = _case(dev, b, v, dtype, strided, kind, seed=v * 29 + b * 11 + ki * 3 + di)
                        f, kw = _tables(logits, df, kind, sampled, done)
                        allowed = f > 0
                        x = logits.float().masked_fill(~allowed, float("-inf"))
                        cols = torch.arange(v, device=dev).expand(b, v)
                        want = torch.where(x == x.max(dim=1, keepdim=True)[0], cols, torch.full_like(cols, v)).min(dim=1)[0]
                        assert bool(allowed.any(dim=1).all()), what                                # no row is left empty
                        tok = K.sample_constrained(logits, 1.0, state=None, finished=done, sample=False, **kw)
                        assert torch.equal(tok.view(-1), want), what
                        if b >= 5:
                            assert int(tok[1]) == kw["pad_code"] and int(allowed[b - 1].sum()) == 1, what
                        pair = torch.empty(2 * b, v + 5 if strided else v, dtype=dtype, device=dev)[:, :v]
                        pair[:b] = logits
                        pair[b:] = (3.0 * torch.randn(b, v, generator=torch.Generator().manual_seed(v + ki))).to(dtype).to(dev)
                        kw2 = dict(kw, forbid_idx=torch.cat([sampled, sampled])) if "forbid_idx" in kw else kw
                        got = K.sample_guided(pair, 1.0, 1.0, state=None, finished=torch.cat([done, done]), sample=False, **kw2)
                        assert torch.equal(got[:b], tok) and torch.equal(got[b:], tok), what
    _bad_rules_are_refused(dev)


def _bad_rules_are_refused(dev):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import DvqError
    for v, pad in ((64, 64), (64, -1), (2049, 0)):
        b = 3
        lg = torch.zeros(b, v, device=dev)
        tg = torch.zeros(b, dtype=torch.int64, device=dev)
        rec = torch.full((b, 2), -1, dtype=torch.int32, device=dev)
        err = torch.zeros(b, dtype=torch.int32, device=dev)
        words = torch.zeros(b * 3, dtype=torch.int32, device=dev)
        state = K.codec_decode_state(words, torch.arange(b, device=dev) * 3, torch.full((b,), 3, device=dev))
        state0 = state.clone()
        calls = {"sample_constrained": lambda: K.sample_constrained(lg, 1.0, pad, None, sample=False),
                 "sample_guided": lambda: K.sample_guided(torch.cat([lg, lg]), 1.0, 1.0, pad, None, sample=False),
                 "codec_tables": lambda: K.codec_tables(lg, pad),
                 "codec_record": lambda: K.codec_record(lg, tg, rec, 0, err, pad),
                 "codec_decode_step": lambda: K.codec_decode_step(lg, state, words, err, pad)}
        for name, call in calls.items():
            with pytest.raises(DvqError):
                call()
                pytest.fail(f"{name} took V = {v}, pad_code = {pad}")
        torch.cuda.synchronize()
        assert bool((rec == -1).all()) and int(err.abs().sum()) == 0 and torch.equal(state, state0), (v, pad)


@pytest.fixture(scope="module")
def long_run(dev):
    """record + encode 300 steps of fresh random logits for 5 rows that finish at different steps (one from the start); shared by the
    round-trip test and the short-count test"""
    from dynamicvectorquantization_amd import kernels as K
    steps, b, v = 300, 5, 515
    df = _rules_model(v)
    kw = _rule_kw(df, "content")
    g = torch.Generator().manual_seed(77)
    finish = torch.tensor([300, 37, 299, 150, 0])
    logits = [(torch.randn(b, v, generator=g) * float(torch.rand(1, generator=g) * 8)).to(dev) for _ in range(steps)]
    for s in (5, 120):                                                                 # steps whose rows have ONE allowed symbol
        row = torch.full((b, v), float("-inf"))
        row[:, 9] = 1.0
        logits[s] = row.to(dev)
    records = torch.zeros(b, steps + 7, dtype=torch.int32, device=dev)
    err = torch.zeros(b, dtype=torch.int32, device=dev)
    targets = []
    for s in range(steps):
        done = (finish <= s).float().view(-1, 1).to(dev)
        f = K.codec_tables(logits[s], finished=done, **kw)
        tg = torch.multinomial((f > 0).float() + f.float() / M, 1).view(-1)
        tok = K.codec_record(logits[s], tg, records, s, err, finished=done, **kw)
        targets.append(tok.view(-1))
    kinds = torch.arange(steps) % 3
    words, nwords, bits = K.codec_encode(records, steps, kinds=kinds.to(dev), want_bits=True)
    return dict(steps=steps, b=b, v=v, kw=kw, finish=finish, logits=logits, records=records, err=err, targets=targets, words=words,
                nwords=nwords, bits=bits, kinds=kinds)


def _decode_all(dev, run, counts):
    from dynamicvectorquantization_amd import kernels as K
    cap = run["words"].shape[1]
    base = torch.arange(run["b"], device=dev) * cap + cap - run["nwords"]             # the buffer itself is kept at full size
    flat = run["words"].reshape(-1).contiguous()
    state = K.codec_decode_state(flat, base, counts)
    err = torch.zeros(run["b"], dtype=torch.int32, device=dev)
    toks = []
    for s in range(run["steps"]):
        done = (run["finish"] <= s).float().view(-1, 1).to(dev)
        toks.append(K.codec_decode_step(run["logits"][s], state, flat, err, finished=done, **run["kw"]).view(-1))
    return toks, state, err


def test_record_encode_decode_300_steps(dev, long_run):
    from dynamicvectorquantization_amd import kernels as K
    run = long_run
    assert int(run["err"].abs().sum()) == 0
    toks, state, err = _decode_all(dev, run, run["nwords"])
    assert int(err.abs().sum()) == 0
    assert torch.equal(torch.stack(toks), torch.stack(run["targets"]))                # decoded tokens == targets
    assert torch.equal(state[:, 0], torch.full((run["b"],), cm.L, dtype=torch.int64, device=dev))       # every final state == L
    assert torch.equal(state[:, 1], run["nwords"])                                    # every cursor == its word count
    words, nwords, recs = run["words"].cpu().numpy().view(np.uint32), run["nwords"].cpu().numpy(), run["records"].cpu().numpy()
    cap = words.shape[1]
    kinds = run["kinds"].numpy()
    for r in range(run["b"]):
        unpacked = cm.unpack_records(recs[r, :run["steps"]])
        ref = cm.rans_encode(unpacked)
        assert ref.tobytes() == words[r, cap - int(nwords[r]):].tobytes(), r          # byte for byte the restatement's stream
        for k in range(3):
            want = cm.ideal_bits([u for u, kk in zip(unpacked, kinds) if kk == k])
            assert abs(float(run["bits"][r, k]) - want) <= 1e-9 * max(1.0, want)
        assert 32 * (int(nwords[r]) - 2) + 64 <= float(run["bits"][r].sum()) + 100    # the overhead bound
    assert int(nwords[4]) == 2                                                        # the row finished from the start: state only
    again = K.codec_encode(run["records"], run["steps"])
    assert torch.equal(again[0], run["words"]) and torch.equal(again[1], run["nwords"])


def test_short_word_count_sets_error_never_reads_past(dev, long_run):
    """row 0's count passed one short of the real one, the buffer itself at full size: the last refill yields zero and sets error
    bit 2 for that row only"""
    run = long_run
    counts = run["nwords"].clone()
    assert int(counts[0]) > 3
    counts[0] -= 1
    toks, state, err = _decode_all(dev, run, counts)
    assert int(err[0]) & 2 and int(err[1:].abs().sum()) == 0
    assert int(state[0, 1]) == int(counts[0])                                         # the cursor stopped at the count


def test_codec_kernels_reject_bad_arguments(dev):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import DvqError
    x = torch.randn(3, 2049, device=dev)
    with pytest.raises(DvqError):
        K.codec_tables(x, pad_code=0)                                                 # V > 2048
    with pytest.raises(DvqError):
        K.codec_tables(x[:, :64], pad_code=64)                                        # pad outside the vocabulary


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ordered_sums(dev):
    """bit-for-bit image comparisons need the first stage's GroupNorm sums in a fixed order (the library's deterministic mode); the
    token round trip itself does not"""
    from dynamicvectorquantization_amd import kernels as K
    was = K.deterministic()
    K.set_deterministic(True)
    yield
    K.set_deterministic(was)


def _group_images(dev):
    """three 64 x 64 images (4 x 4 cells): all flat (coarse), all noise (fine), and a mixed one whose last cell is flat"""
    from dynamicvectorquantization_amd import synth
    seed = next(s for s in range(1, 200) if synth.half_flat_layout(1, 64, 16, s, 0.5)[0, -1, -1] == synth.half_flat_layout(
        1, 64, 16, s, 0.0)[0, -1, -1])
    x = np.concatenate([synth.half_flat_images(1, 64, seed=3, fine_fraction=0.0), synth.half_flat_images(1, 64, seed=4, fine_fraction=1.0),
                        synth.half_flat_images(1, 64, seed=seed, fine_fraction=0.5)])
    return torch.from_numpy(x).to(dev)


def _model(dev, kind):
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from test_gpu_guidance import class_config
    from test_gpu_stage2 import dualformer_config
    torch.manual_seed(1)
    model = instantiate_from_config(dualformer_config() if kind == "uncond" else class_config()).to(dev).eval()
    with torch.no_grad():                      # random weights, the heads scaled up: peaked next-token distributions, not uniform ones
        model.transformer.content_head[1].weight.mul_(40.0)
        model.transformer.position_head[1].weight.mul_(40.0)
    rt.bump_weights_epoch()
    return model


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["uncond", "class"])
def test_compress_decompress_round_trip(dev, ordered_sums, kind, dtype):
    from dynamicvectorquantization_amd import codec
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(dtype), torch.no_grad():
        model = _model(dev, kind)
        x = _group_images(dev)
        labels = torch.tensor([3, 0, 9], device=dev) if kind == "class" else None
        enc = model.first_stage_model.encode(x)
        indices, grain = enc[2][2].reshape(3, model.fine_hw, model.fine_hw).long(), enc[3].reshape(3, model.hw1, model.hw1).long()
        assert int(grain[0].sum()) == 0 and int(grain[1].sum()) == model.hw1 ** 2            # all coarse; all fine
        assert 0 < int(grain[2].sum()) < model.hw1 ** 2 and int(grain[2, -1, -1]) == 0        # mixed, cell hw1^2 - 1 coarse
        cond = model.encode_to_c(labels if kind == "class" else x)
        sample_kw = dict(temperature=1.0, sample=True, top_k=100, top_k_pos=10, fix_fine_position=True)

        def sample():
            # the draws' device generator {seed, counter} continues across calls under one torch seed: restart it, so that the two
            # calls differ in nothing but what ran between them
            torch.manual_seed(11)
            model.__dict__.pop("_sampler_state", None)
            return model.sample_from_scratch(*cond, **sample_kw)

        before = sample()

        blob, bits = model.compress(x, labels, batch_group=3, return_bits=True)
        assert isinstance(blob, bytes) and bits.shape == (3, 3) and bits.dtype == torch.float64
        assert model.compress(x, labels, batch_group=3) == blob                              # compressing twice: identical bytes
        got_idx, got_grain = model.decompress(blob)
        assert torch.equal(got_grain, grain)
        assert torch.equal(got_idx, indices)
        _, z = model.encode_to_z(x)
        want_img = model.decode_to_img(z["coarse_content"], z["fine_content"], z["coarse_position"], z["fine_position"])
        assert torch.equal(model.decompress_images(blob), want_img)
        payload = codec.payload_bits(blob)
        ideal = bits.sum(dim=1).cpu().numpy()
        print(f"{kind} {dtype}: payload bits {payload.tolist()}, ideal {np.round(ideal, 1).tolist()}")
        assert (payload <= ideal + 100).all()             # payload = 32 x renormalisation words + 64 (the two state words)
        assert float(bits[0, 2]) == 0.0 and float(bits[1, 1]) == 0.0                         # all coarse: no fine content; all fine: no coarse
        assert float(bits[2].min()) > 0.0

        # other groupings decode too, and a group of one differs from the group of three only in its bytes
        blob1 = model.compress(x, labels, batch_group=2)
        idx1, grain1 = model.decompress(blob1)
        assert torch.equal(idx1, indices) and torch.equal(grain1, grain)

        header, groups = codec.parse_container(blob)
        with pytest.raises(codec.CodecError, match="fingerprint"):
            other = bytearray(blob)
            other[24] ^= 0xFF
            other[36:40] = np.asarray([zlib.crc32(bytes(other[:36]))], dtype="<u4").tobytes()
            model.decompress(bytes(other))
        with pytest.raises(codec.CodecError):
            model.decompress(blob[:-5])
        if kind == "class":
            # wrong labels in an otherwise valid container (CRC recomputed): other tokens or a CodecError, and it terminates
            wrong = [(np.asarray([7, 7, 1], dtype=np.int32), words) for _, words in groups]
            patched = codec.pack_container(wrong, header["group_size"], header["fingerprint"], codec.DTYPE_CODES[header["dtype"]],
                                           header["step"], header["coarse_hw"], header["fine_hw"], True)
            # a label outside [0, n_classes) would become a gather index on the device: refused on the host, force or not
            for bad_label in (model.n_classes, -1, 2 ** 31 - 1):
                evil = [(np.asarray([3, bad_label, 9], dtype=np.int32), words) for _, words in groups]
                evil_blob = codec.pack_container(evil, header["group_size"], header["fingerprint"], codec.DTYPE_CODES[header["dtype"]],
                                                 header["step"], header["coarse_hw"], header["fine_hw"], True)
                for force in (False, True):
                    with pytest.raises(codec.CodecError, match="class label"):
                        model.decompress(evil_blob, force=force)
                with pytest.raises(codec.CodecError, match="class label"):
                    model.compress(x, torch.tensor([3, bad_label, 9], device=dev), batch_group=3)
            try:
                bad_idx, bad_grain = model.decompress(patched)
                assert not (torch.equal(bad_idx, indices) and torch.equal(bad_grain, grain))
            except codec.CodecError:
                pass
        else:
            with pytest.raises(codec.CodecError, match="labels"):                           # a labelled container, a model without
                model.decompress(codec.pack_container(
                    [(np.zeros(3, dtype=np.int32), groups[0][1])], 3, header["fingerprint"], codec.DTYPE_CODES[header["dtype"]],
                    header["step"], header["coarse_hw"], header["fine_hw"], True))

        after = sample()
        assert all(torch.equal(a, b) for a, b in zip(before, after))                         # no state leaks into the sampler


def test_compress_tokens_and_wrong_dtype(dev, ordered_sums):
    """compress_tokens codes stored streams to the same bytes as compress; a bf16 stream under fp32 compute is refused unless forced"""
    from dynamicvectorquantization_amd import codec
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    with torch.no_grad():
        with rt.compute_dtype_ctx(torch.bfloat16):
            model = _model(dev, "uncond")
            x = _group_images(dev)
            _, z = model.encode_to_z(x)
            blob = model.compress_tokens(z, batch_group=3)
            assert blob == model.compress(x, batch_group=3)
            # the recording loop and the decoding loop take no launch whose sum depends on arrival order, by the library's own count
            K.set_deterministic(False)                                                        # (the count only moves with the mode off)
            try:
                n0 = K.unordered_launches()
                assert model.compress_tokens(z, batch_group=3) == blob
                codec.decompress_tokens(model, blob)
                assert K.unordered_launches() == n0
            finally:
                K.set_deterministic(True)
            bad = {k: v.clone() for k, v in z.items()}
            bad["coarse_content"][2, 0] = model.content_eos_code                              # a token the rule forbids
            with pytest.raises(codec.CodecError, match="forbids"):
                model.compress_tokens(bad, batch_group=3)
        with rt.compute_dtype_ctx(torch.float32):
            with pytest.raises(codec.CodecError, match="compute dtype"):
                model.decompress(blob)
