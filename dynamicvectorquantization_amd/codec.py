"""Lossless token codec: rANS-code images with the DQ-Transformer as the entropy model (docs/design/27-token-codec.md).

`Dualformer.compress` / `decompress` (stage2.py) land here.  Encoding is the K/V-cached sampler loop (`_sample_cached`,
fix_fine_position=True) with the image's own tokens forced in and (cum, f) of each recorded (kernels.codec_record); one kernel then
walks each image's records backwards (kernels.codec_encode).  Decoding is the same loop with the bitstream in place of the random
generator (kernels.codec_decode_step).  An image's logits depend on its batch mates, so the unit of coding is a GROUP: the images
that went through the loop together; the decoder re-forms exactly those groups.

The container half of this module (pack / parse / CodecError) needs numpy only: the host rejects a damaged or foreign blob before
anything reaches the GPU (class labels included: they index embedding tables).  A stream is tied to the checkpoint, the compute
dtype, the kernels of the build that wrote it, and whatever selects the token step's summation layout: the device's CU count and the
DVQ_DECODE_* switches (docs/design/27-token-codec.md, Determinism).

Container, little-endian:
    header (40 bytes)
        0   4s  magic b"DQTC"
        4   H   version (1)
        6   B   compute dtype: 0 fp32, 1 bf16, 2 fp32x3
        7   B   token step: 0 one kernel per operation, 1 the fused per-transformer kernel (DecodeState._stack)
        8   I   group size G (images per group; the last group may hold fewer)
        12  I   number of images N
        16  B   1 if class labels travel with the groups, else 0
        17  B   reserved (0)
        18  H   coarse_hw
        20  H   fine_hw
        22  H   reserved (0)
        24  8s  model fingerprint
        32  I   reserved (0)
        36  I   CRC-32 of bytes 0 .. 36
    per group, ceil(N / G) of them
        I       n = images in the group
        n x i   class labels (only with labels)
        n x I   words per image (each >= 2)
        words   the images' word streams, one after the other, uint32 each
        I       CRC-32 of the group's bytes up to here
"""
from __future__ import annotations

import hashlib
import struct
import zlib

import numpy as np

MAGIC = b"DQTC"
VERSION = 1
HEADER = struct.Struct("<4sHBBIIBBHHH8sI")
HEADER_BYTES = HEADER.size + 4
DTYPE_CODES = {"fp32": 0, "bf16": 1, "fp32x3": 2}
DTYPE_NAMES = {v: k for k, v in DTYPE_CODES.items()}
MAX_GROUP = 1 << 16


class CodecError(RuntimeError):
    """a blob that is not a token container, is damaged, belongs to another model / dtype, or does not decode"""


# ---------------------------------------------------------------------------------------------
# container (numpy only)
# ---------------------------------------------------------------------------------------------
def pack_container(groups, group_size, fingerprint, dtype_code, step_code, coarse_hw, fine_hw, with_labels):
    """groups: list of (labels int array [n] or None, list of n uint32 arrays) -> bytes"""
    n_images = sum(len(words) for _, words in groups)
    assert len(fingerprint) == 8 and 1 <= group_size <= MAX_GROUP
    head = HEADER.pack(MAGIC, VERSION, dtype_code, step_code, group_size, n_images, int(bool(with_labels)), 0, coarse_hw, fine_hw, 0,
                       bytes(fingerprint), 0)
    out = [head, struct.pack("<I", zlib.crc32(head) & 0xFFFFFFFF)]
    for labels, words in groups:
        n = len(words)
        parts = [struct.pack("<I", n)]
        if with_labels:
            parts.append(np.asarray(labels, dtype="<i4").reshape(n).tobytes())
        parts.append(np.asarray([len(w) for w in words], dtype="<u4").tobytes())
        parts.extend(np.ascontiguousarray(w, dtype="<u4").tobytes() for w in words)
        body = b"".join(parts)
        out.append(body)
        out.append(struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF))
    return b"".join(out)


def parse_container(blob, max_words_per_image=None):
    """-> (header dict, groups = list of (labels int32 [n] or None, list of n uint32 arrays)).  Validates magic, version, every count
    and every CRC; raises CodecError on the first thing that is off.  Nothing here touches the GPU."""
    blob = bytes(blob)
    if len(blob) < HEADER_BYTES:
        raise CodecError(f"truncated container: {len(blob)} bytes, the header alone has {HEADER_BYTES}")
    (magic, version, dtype_code, step_code, group_size, n_images, with_labels, _r0, coarse_hw, fine_hw, _r1, fingerprint,
     _r2) = HEADER.unpack_from(blob, 0)
    if magic != MAGIC:
        raise CodecError(f"bad magic {magic!r}: not a token container")
    if version != VERSION:
        raise CodecError(f"container version {version}; this build reads version {VERSION}")
    (crc,) = struct.unpack_from("<I", blob, HEADER.size)
    if crc != (zlib.crc32(blob[:HEADER.size]) & 0xFFFFFFFF):
        raise CodecError("header CRC mismatch")
    if dtype_code not in DTYPE_NAMES or step_code not in (0, 1) or with_labels not in (0, 1):
        raise CodecError("header holds an unknown dtype / token-step / label code")
    if not 1 <= group_size <= MAX_GROUP:
        raise CodecError(f"group size {group_size} out of range")
    header = dict(dtype=DTYPE_NAMES[dtype_code], step=step_code, group_size=group_size, n_images=n_images, with_labels=bool(with_labels),
                  coarse_hw=coarse_hw, fine_hw=fine_hw, fingerprint=fingerprint)
    if max_words_per_image is None:
        max_words_per_image = 2 * coarse_hw * coarse_hw + fine_hw * fine_hw + 8           # steps of the loop + 2, with slack
    groups, off, left = [], HEADER_BYTES, n_images
    while left > 0:
        start = off
        if off + 4 > len(blob):
            raise CodecError("truncated container: a group header is missing")
        (n,) = struct.unpack_from("<I", blob, off)
        off += 4
        if n != min(group_size, left):
            raise CodecError(f"group of {n} images where {min(group_size, left)} are due")
        need = (4 * n if with_labels else 0) + 4 * n
        if off + need > len(blob):
            raise CodecError("truncated container: group counts are missing")
        labels = None
        if with_labels:
            labels = np.frombuffer(blob, dtype="<i4", count=n, offset=off).astype(np.int32)
            off += 4 * n
        counts = np.frombuffer(blob, dtype="<u4", count=n, offset=off).astype(np.int64)
        off += 4 * n
        if (counts < 2).any() or (counts > max_words_per_image).any():
            raise CodecError(f"word count outside [2, {max_words_per_image}]")
        total = int(counts.sum())
        if off + 4 * total + 4 > len(blob):
            raise CodecError("truncated container: word streams are missing")
        words, at = [], off
        for k in counts.tolist():
            words.append(np.frombuffer(blob, dtype="<u4", count=k, offset=at).astype(np.uint32))
            at += 4 * k
        off = at
        (crc,) = struct.unpack_from("<I", blob, off)
        if crc != (zlib.crc32(blob[start:off]) & 0xFFFFFFFF):
            raise CodecError(f"CRC mismatch in group {len(groups)}")
        off += 4
        groups.append((labels, words))
        left -= n
    if off != len(blob):
        raise CodecError(f"{len(blob) - off} bytes after the last group")
    return header, groups


def check_header(header, fingerprint, dtype, step_code, coarse_hw, fine_hw, with_labels, force=False):
    """the parsed header against the model that is about to decode; force=True lets a foreign fingerprint, dtype or token step pass"""
    if (header["coarse_hw"], header["fine_hw"]) != (coarse_hw, fine_hw):
        raise CodecError(f"container geometry {header['coarse_hw']} / {header['fine_hw']}, model {coarse_hw} / {fine_hw}")
    if header["with_labels"] != bool(with_labels):
        raise CodecError("class labels: the container and the model disagree on whether there are any")
    if force:
        return
    if header["fingerprint"] != bytes(fingerprint):
        raise CodecError(f"model fingerprint {bytes(fingerprint).hex()} does not match the container's {header['fingerprint'].hex()} "
                         "(a stream decodes only under the checkpoint that wrote it; force=True tries anyway)")
    if header["dtype"] != dtype:
        raise CodecError(f"container written in {header['dtype']}, the compute dtype is {dtype} (force=True tries anyway)")
    if header["step"] != step_code:
        raise CodecError("container written by the other token-step kernel variant (DVQ_DECODE_STACK; force=True tries anyway)")


def check_labels(labels, n_classes):
    """class labels become embedding-table rows (label + threshold, ClassAwareSOSProvider) that the device gathers without a bounds
    check: every label must lie in [0, n_classes) before it leaves the host.  labels: integer array or None"""
    if labels is None:
        return
    lab = np.asarray(labels).reshape(-1)
    if n_classes is None:
        raise CodecError("class labels given, but the model does not say how many classes it has (n_classes)")
    if lab.size and (int(lab.min()) < 0 or int(lab.max()) >= int(n_classes)):
        bad = lab[(lab < 0) | (lab >= int(n_classes))]
        raise CodecError(f"class label {int(bad[0])} outside [0, {int(n_classes)})")


def payload_bits(blob):
    """per image: 32 x words of its stream (the container's framing not counted) -> int64 [N]"""
    _, groups = parse_container(blob)
    return np.asarray([32 * len(w) for _, words in groups for w in words], dtype=np.int64)


# ---------------------------------------------------------------------------------------------
# model side
# ---------------------------------------------------------------------------------------------
def model_fingerprint(model):
    """8 bytes: SHA-256 over the transformer's and the first stage's parameter bytes in state_dict order; computed once per model
    object and cached on it, keyed by every parameter's (storage, version counter): load_state_dict or an optimizer step on the same
    object bumps the counters and the next call hashes again"""
    import torch
    key = tuple((p_.data_ptr(), p_._version) for part in (model.transformer, model.first_stage_model) for p_ in part.parameters())
    cached = model.__dict__.get("_codec_fingerprint")
    fp = cached[1] if cached is not None and cached[0] == key else None
    if fp is None:
        h = hashlib.sha256()
        for part in (model.transformer, model.first_stage_model):
            names = {n for n, _ in part.named_parameters()}
            for name, t in part.state_dict().items():
                if name in names:
                    h.update(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes())
        fp = h.digest()[:8]
        model.__dict__["_codec_fingerprint"] = (key, fp)
    return fp


def _dtype_name():
    import torch
    from . import runtime as rt
    if rt.compute_dtype() == torch.bfloat16:
        return "bf16"
    return "fp32x3" if rt.fp32_split() else "fp32"


def codec_rule(model, kind):
    """the sampler's rule for `kind` (`_fused_rule`, with the ClassDualformer overrides) with one change: coarse positions are
    forbidden from the pad code on, not from cell hw1^2 - 1 on -- real images use the last cell"""
    kw = model._fused_rule(kind)
    if kind == "coarse_pos":
        kw["forbid_from"] = model.coarse_position_pad_code
    return kw


class _CodecSource:
    """a token source of `_sample_cached` (see stage2._SampleSource): loop caps and rule marshalling shared by record and decode"""

    def __init__(self, model, batch, dev):
        import torch
        self.model = model
        self.max_coarse_steps = model.hw1 * model.hw1 + 1              # every cell once, then <eos>: whatever the stream says
        self.max_steps = 2 * self.max_coarse_steps + model.fine_hw * model.fine_hw + 2
        self.err = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.rules = {k: codec_rule(model, k) for k in ("coarse_pos", "fine_pos", "content")}
        self.step = 0
        self.decode_state = None                                       # the DecodeState the loop ran on (set by _sample_cached)

    def _rule(self, logits2d, rule):
        from . import kernels as K
        from .stage2 import rule_kwargs
        kind, sampled, done = rule
        if not K.token_rule_ok(logits2d):
            raise CodecError("the codec needs device logits, fp32 or bf16, within the column limit of its kernels (kernels.token_rule_ok)")
        if self.step >= self.max_steps:
            raise CodecError("the token loop ran past its step capacity")
        return rule_kwargs(self.rules[kind], kind, sampled), done

    def check(self):
        """the device error words, read once per group"""
        from .kernels import CODEC_ERRORS
        bits = self.err.cpu().numpy()
        if bits.any():
            what = sorted({msg for b, msg in CODEC_ERRORS.items() if (bits & b).any()})
            raise CodecError(f"images {np.nonzero(bits)[0].tolist()} of the group: " + "; ".join(what))


class RecordSource(_CodecSource):
    """encode: the image's own tokens are forced in, (cum, f) of each is recorded"""

    def __init__(self, model, z):
        import torch
        cc = z["coarse_content"]
        super().__init__(model, cc.shape[0], cc.device)
        self.targets = (z["coarse_position"].long(), cc.long(), z["fine_content"].long())
        self.records = torch.zeros(cc.shape[0], self.max_steps, dtype=torch.int32, device=cc.device)
        self.kinds = []
        self.n_pos = self.n_con = 0

    def token(self, logits2d, rule):
        from . import kernels as K
        kw, done = self._rule(logits2d, rule)
        if rule[0] == "coarse_pos":
            stream, at = 0, self.n_pos
            self.n_pos += 1
        elif rule[0] == "content":                  # coarse content follows its position draw; fine content comes after all of them
            stream, at = (1, self.n_con) if self.n_con < self.n_pos else (2, self.n_con - self.n_pos)
            self.n_con += 1
        else:
            raise CodecError("fine positions are not coded (fix_fine_position=True)")
        tg = self.targets[stream]
        if at >= tg.shape[1]:
            raise CodecError("the token streams are shorter than the loop they drive (inconsistent tokens)")
        out = K.codec_record(logits2d, tg[:, at], self.records, self.step, self.err, finished=done, **kw)
        self.kinds.append(stream)
        self.step += 1
        return out


class DecodeSource(_CodecSource):
    """decode: the bitstream replaces the random generator"""

    def __init__(self, model, words, dev):
        import torch
        from . import kernels as K
        super().__init__(model, len(words), dev)
        counts = torch.tensor([len(w) for w in words], dtype=torch.int64)
        base = torch.cumsum(counts, 0) - counts
        flat = np.concatenate(words).astype(np.uint32)
        self.words = torch.from_numpy(flat.view(np.int32).copy()).to(dev)
        self.state = K.codec_decode_state(self.words, base.to(dev), counts.to(dev))
        self.counts = counts

    def token(self, logits2d, rule):
        from . import kernels as K
        if rule[0] == "fine_pos":
            raise CodecError("fine positions are not coded (fix_fine_position=True)")
        kw, done = self._rule(logits2d, rule)
        self.step += 1
        return K.codec_decode_step(logits2d, self.state, self.words, self.err, finished=done, **kw)

    def check(self):
        super().check()
        st = self.state.cpu()
        if not bool((st[:, 0] == (1 << 31)).all()) or not bool((st[:, 1] == self.counts).all()):
            raise CodecError("a word stream did not end where its tokens did: a damaged stream, or one written under another model, "
                             "dtype, build, device (CU count / partition) or DVQ_DECODE_* setting")


class _eval_mode:
    """the transformer in eval mode (no dropout; the cached sampler path) whatever mode it is in, every flag put back as found"""

    def __init__(self, model):
        self.on = [m for m in model.transformer.modules() if m.training]

    def __enter__(self):
        for m in self.on:
            m.training = False

    def __exit__(self, *exc):
        for m in self.on:
            m.training = True


def _run_loop(model, cond, source):
    """`_sample_cached` with `source` in place of the draws (it reads the source's error words next to DecodeState.check);
    -> (x_c, x_f, x_pc, x_pf, token-step code of the DecodeState used)"""
    from ._lib import DvqError
    try:
        out = model._sample_cached(*cond, 1.0, True, None, None, None, None, True, None, source=source)
    except AssertionError as e:                      # DecodeState's row capacity
        raise CodecError(f"token loop left the decode state's capacity: {e}") from e
    except DvqError as e:
        raise CodecError(str(e)) from e
    st = source.decode_state
    return out + (int(st is not None and any(k in st._stacks for k in ("pos", "con"))),)


def _conditioning(model, c, like):
    """the six start-token tensors of a group: c = class labels (ClassDualformer) or nothing (the start tokens only need a batch)"""
    if model.cond_stage_key == model.first_stage_key:
        return model.encode_to_c(like)
    if c is None:
        raise CodecError("a class-conditional model codes with class labels: pass c")
    c = c.reshape(-1).long()
    check_labels(c.cpu().numpy(), getattr(model, "n_classes", None))          # (on the host: the device gathers rows by them)
    return model.encode_to_c(c.to(like.device))


def compress_tokens(model, tokens, c=None, batch_group=8, return_bits=False):
    """rANS-code stored token streams (`tokens` = the permuter's dict of B images) -> bytes [, ideal bits fp64 [B, 3]]"""
    import torch
    from . import kernels as K
    cc_all = tokens["coarse_content"]
    b, dev = cc_all.shape[0], cc_all.device
    batch_group = max(1, min(int(batch_group), MAX_GROUP))
    with_labels = model.cond_stage_key != model.first_stage_key
    groups, bits_all, step_codes = [], [], set()
    eos_c, eos_f = model.coarse_position_eos_code, model.fine_position_eos_code
    with torch.no_grad(), _eval_mode(model):
        for g0 in range(0, b, batch_group):
            sl = slice(g0, min(b, g0 + batch_group))
            z = {k: tokens[k][sl] for k in ("coarse_content", "coarse_position", "fine_content", "fine_position")}
            # trim to the group's own longest streams: the loop's length is the group's, not the batch's
            lc = int((torch.cumsum((z["coarse_position"] == eos_c).long(), 1) == 0).sum(dim=1).max()) + 1
            lf = int((torch.cumsum((z["fine_position"] == eos_f).long(), 1) == 0).sum(dim=1).max()) + 1
            if not bool((z["coarse_position"] == eos_c).any(dim=1).all()) or not bool((z["fine_position"] == eos_f).any(dim=1).all()):
                raise CodecError("a token stream has no <eos>")
            z = {k: (v[:, :lc] if k.startswith("coarse") else v[:, :lf]).contiguous() for k, v in z.items()}
            labels = None if c is None else c.reshape(-1)[sl]
            cond = _conditioning(model, labels, z["coarse_content"])
            src = RecordSource(model, z)
            x_c, x_f, x_pc, x_pf, step_code = _run_loop(model, cond, src)
            if x_pc.shape != z["coarse_position"].shape or x_pf.shape != z["fine_position"].shape or \
                    not torch.equal(x_pf, z["fine_position"]):
                raise CodecError("the fine positions do not follow from the coarse ones in the permuter's order (inconsistent tokens)")
            kinds = torch.tensor(src.kinds, dtype=torch.uint8, device=dev)
            words, nwords, bits = K.codec_encode(src.records, src.step, kinds=kinds, want_bits=True)
            cap = words.shape[1]
            w_host, n_host = words.cpu().numpy().view(np.uint32), nwords.cpu().numpy()
            groups.append((None if not with_labels else labels.cpu().numpy().astype(np.int32),
                           [w_host[i, cap - int(n_host[i]):].copy() for i in range(w_host.shape[0])]))
            bits_all.append(bits)
            step_codes.add(step_code)
    if len(step_codes) > 1:
        raise CodecError("the token-step kernel variant changed between groups (a barrier time-out switched the fused kernel off)")
    blob = pack_container(groups, batch_group, model_fingerprint(model), DTYPE_CODES[_dtype_name()], step_codes.pop() if step_codes else 0,
                          model.hw1, model.fine_hw, with_labels)
    if return_bits:
        return blob, (torch.cat(bits_all) if bits_all else torch.zeros(0, 3, dtype=torch.float64, device=dev))
    return blob


def compress(model, x, c=None, batch_group=8, return_bits=False):
    """rANS-code the images x [B, 3, H, W] (c: class labels for the class-conditional model) -> bytes [, ideal bits fp64 [B, 3] by
    stream: coarse position, coarse content, fine content].  Each group of `batch_group` images is tokenised and coded together."""
    import torch
    batch_group = max(1, min(int(batch_group), MAX_GROUP))
    with torch.no_grad():
        zs = [model.encode_to_z(x[g0:g0 + batch_group])[1] for g0 in range(0, x.shape[0], batch_group)]
    return compress_tokens(model, cat_tokens(model, zs), c, batch_group, return_bits)


def cat_tokens(model, zs):
    """the permuter dicts of several batches as one: every stream padded with its pad code to the longest batch's width"""
    import torch
    pad = {"coarse_content": model.content_pad_code, "fine_content": model.content_pad_code,
           "coarse_position": model.coarse_position_pad_code, "fine_position": model.fine_position_pad_code}
    width = {k: max(z[k].shape[1] for z in zs) for k in pad}
    return {k: torch.cat([torch.nn.functional.pad(z[k], (0, width[k] - z[k].shape[1]), value=pad[k]) for z in zs]) for k in pad}


def decompress_tokens(model, blob, force=False, device=None):
    """-> (coarse_content, fine_content, coarse_position, fine_position) lists per group, after every host-side check"""
    import torch
    header, groups = parse_container(blob)
    with_labels = model.cond_stage_key != model.first_stage_key
    dev = device if device is not None else next(model.transformer.parameters()).device
    # the token-step variant is only known once a DecodeState has run (it may fall back from the fused kernel), so the header's own
    # code is passed here and the real comparison follows the first group's loop below
    check_header(header, model_fingerprint(model), _dtype_name(), header["step"], model.hw1, model.fine_hw, with_labels, force)
    if with_labels:                                  # every group's labels before ANY group reaches the GPU; force does not lift this
        for labels, _ in groups:
            check_labels(labels, getattr(model, "n_classes", None))
    out = []
    with torch.no_grad(), _eval_mode(model):
        for labels, words in groups:
            like = torch.zeros(len(words), 1, dtype=torch.long, device=dev)
            cond = _conditioning(model, None if labels is None else torch.from_numpy(labels.astype(np.int64)), like)
            src = DecodeSource(model, words, dev)
            x_c, x_f, x_pc, x_pf, step_code = _run_loop(model, cond, src)
            if step_code != header["step"] and not force:
                raise CodecError("container written by the other token-step kernel variant (DVQ_DECODE_STACK; force=True tries anyway)")
            out.append((x_c, x_f, x_pc, x_pf, cond))
    return out


def decompress(model, blob, force=False):
    """-> (indices int64 [N, fine_hw, fine_hw], grain_indices int64 [N, coarse_hw, coarse_hw]): what encode_to_z saw"""
    return codes_of(model, decompress_tokens(model, blob, force))


def codes_of(model, decoded):
    """(indices, grain_indices) of what decompress_tokens returned"""
    import torch
    idx, grain = [], []
    for x_c, x_f, x_pc, x_pf, cond in decoded:
        idx.append(model.permuter.forward_back(x_c, x_f, x_pc, x_pf))
        grain.append(1 - model._coarse_cells_drawn(torch.cat([cond[2], x_pc], dim=1)))
    dev = next(model.transformer.parameters()).device
    if not idx:
        return (torch.zeros(0, model.fine_hw, model.fine_hw, dtype=torch.long, device=dev),
                torch.zeros(0, model.hw1, model.hw1, dtype=torch.long, device=dev))
    return torch.cat(idx), torch.cat(grain)


def images_of(model, decoded):
    """decode_to_img of what decompress_tokens returned, group by group -> [N, 3, H, W] (None without images)"""
    import torch
    imgs = [model.decode_to_img(x_c, x_f, x_pc, x_pf) for x_c, x_f, x_pc, x_pf, _ in decoded]
    return torch.cat(imgs) if imgs else None


def decompress_images(model, blob, force=False):
    """-> images [N, 3, H, W]: decode_to_img of the decoded token streams, group by group"""
    return images_of(model, decompress_tokens(model, blob, force))
