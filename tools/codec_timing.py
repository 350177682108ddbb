#!/usr/bin/env python3
"""Speed of the lossless token codec next to the sampler whose loop it shares (docs/design/27-token-codec.md).

At configs/stage2/uncond_imagenet_p6c18.yml with random weights (256 x 256 synthetic images, half of the cells fine), per batch size:
Dualformer.compress_tokens (the recording loop + the rANS pass), codec.decompress_tokens (the decoding loop) and
sample_from_scratch(fix_fine_position=True) at the same batch, in alternating rounds after a warm-up, wall clock around a
synchronise (each loop reads its `done` flags on the host every coarse step anyway).  A token step is one drawn (or coded) token of
one image.  The sampler draws its own stream lengths, and a fine token costs two transformer passes for one draw (its position is
given) where a coarse token costs one pass per draw; what compares between the loops is therefore the time per transformer pass
(2 x (coarse rows + fine rows) passes per loop).  A coarse iteration (two passes, two draws, one host read of `done`) costs several
fine iterations, and the sampler's stream mix is its own: the row "sampler draws, the images' streams" runs the sampler's draw kernel at
every step but feeds the images' tokens, i.e. the sampler's cost on exactly the streams the codec walks.  Writes the table to --out.

    python tools/codec_timing.py --out profiles/codec_timing.txt
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,50")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import torch

    from dynamicvectorquantization_amd import codec
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.stage2 import _SampleSource
    dev = torch.device("cuda:0")

    class ForcedDraws(_SampleSource):
        """the sampler's draw at every step (its kernel, its host work), the images' own tokens fed onwards"""

        def __init__(self, model, z):
            super().__init__(model, 1.0, True, 300, None, 50, None, None)
            self.streams, self.n_pos, self.n_con = (z["coarse_position"], z["coarse_content"], z["fine_content"]), 0, 0

        def token(self, logits2d, rule):
            super().token(logits2d, rule)
            if rule[0] == "coarse_pos":
                k, at = 0, self.n_pos
                self.n_pos += 1
            else:
                k, at = (1, self.n_con) if self.n_con < self.n_pos else (2, self.n_con - self.n_pos)
                self.n_con += 1
            return self.streams[k][:, at:at + 1].contiguous()

    rt.set_compute_dtype(opt.dtype)
    yml = os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml")
    model, size = E.load_stage2_model(yml, "", dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    lines = [f"token codec against the sampler, uncond_imagenet_p6c18.yml, random weights, {opt.dtype}, {size} x {size} images, "
             f"{torch.cuda.get_device_name(0)} (tools/codec_timing.py; wall clock around a synchronise, after a warm-up, {opt.rounds} "
             "alternating rounds; token-steps/s = drawn or coded tokens of all images per second; a pass = one single-row step of one "
             "of the two transformers for the whole batch)", ""]
    with torch.no_grad():
        for bs in [int(v) for v in opt.batches.split(",")]:
            x = torch.from_numpy(synth.half_flat_images(bs, size, seed=900 + bs)).to(dev)
            _, z = model.encode_to_z(x)
            cond = model.encode_to_c(x)

            def enc():
                return model.compress_tokens(z, batch_group=bs, return_bits=True)

            def sample():
                return model.sample_from_scratch(*cond, temperature=1.0, sample=True, top_k=300, top_k_pos=50, fix_fine_position=True)

            def forced():
                return model._sample_cached(*cond, 1.0, True, 300, None, 50, None, True, None, source=ForcedDraws(model, z))

            blob, bits = enc()
            dec = lambda: codec.decompress_tokens(model, blob)
            dec(), sample(), forced()                             # warm-up: the token-step graphs of this batch size
            enc_steps = 2 * z["coarse_position"].shape[1] + z["fine_position"].shape[1]
            enc_pass = 2 * (z["coarse_position"].shape[1] + z["fine_position"].shape[1])
            te, td, ts, tf, sample_steps, sample_pass = [], [], [], [], [], []
            for _ in range(opt.rounds):
                te.append(timed(enc)[0])
                t, out = timed(dec)
                td.append(t)
                assert torch.equal(out[0][2], z["coarse_position"]) and torch.equal(out[0][3], z["fine_position"])
                assert torch.equal(model.permuter.forward_back(*out[0][:4]), model.permuter.forward_back(
                    z["coarse_content"], z["fine_content"], z["coarse_position"], z["fine_position"]))
                t, out = timed(sample)
                ts.append(t)
                sample_steps.append(2 * out[2].shape[1] + out[3].shape[1])
                sample_pass.append(2 * (out[2].shape[1] + out[3].shape[1]))
                tf.append(timed(forced)[0])
            payload = codec.payload_bits(blob)
            ideal = bits.sum(dim=1).cpu().numpy()
            rate = lambda t, steps: f"{min(t) * 1e3:9.1f} ms  {bs / min(t):8.1f} images/s  {bs * steps / min(t):9.0f} token-steps/s"
            per_pass_s = [t / p_ for t, p_ in zip(ts, sample_pass)]
            spread = lambda v: (max(v) - min(v)) / min(v)
            k = sample_steps[ts.index(min(ts))]
            per_e, per_d, per_s = min(te) / enc_pass, min(td) / enc_pass, min(per_pass_s)
            lines += [
                f"batch {bs} (one group; {enc_steps} token steps per image in {enc_pass} passes; the sampler drew {sample_steps} in "
                f"{sample_pass} passes):",
                f"  compress_tokens (record + rANS pass)   {rate(te, enc_steps)}   rounds {['%.1f' % (v * 1e3) for v in te]}",
                f"  decompress_tokens                      {rate(td, enc_steps)}   rounds {['%.1f' % (v * 1e3) for v in td]}",
                f"  sample_from_scratch(fix_fine_position) {rate(ts, k)}   rounds {['%.1f' % (v * 1e3) for v in ts]}",
                f"  sampler draws, the images' streams     {rate(tf, enc_steps)}   rounds {['%.1f' % (v * 1e3) for v in tf]}",
                f"  on the same streams: encode / sampler draws {min(te) / min(tf):.3f}, decode / sampler draws {min(td) / min(tf):.3f}; "
                f"spread of the sampler-draw rounds {spread(tf):.1%}",
                f"  per transformer pass: encode {per_e * 1e6:.1f} us, decode {per_d * 1e6:.1f} us, sample {per_s * 1e6:.1f} us; encode / "
                f"sample {per_e / per_s:.3f}, decode / sample {per_d / per_s:.3f}; round-to-round spread encode {spread(te):.1%}, decode "
                f"{spread(td):.1%}, sample (per pass) {spread(per_pass_s):.1%}",
                f"  bytes per image {payload.mean() / 8:.1f} (container {len(blob) / bs:.1f}), ideal {ideal.mean() / 8:.1f}, overhead "
                f"{(payload - ideal).mean():.1f} bits per image",
                ""]
    # the draw kernels alone, at the content head's shape: HIP events over back-to-back calls (GPU time per call when the GPU is the
    # bottleneck) and the host clock over the same calls (what a call costs the launching thread)
    from dynamicvectorquantization_amd import kernels as K
    v = model.transformer.config.vocab_size
    lines.append(f"draw kernels alone, fp32 logits [B, {v}], content rule, 300 back-to-back calls (HIP events / host clock, us per call):")
    for bs in [int(b_) for b_ in opt.batches.split(",")]:
        lg = torch.randn(bs, v, device=dev) * 3
        done = torch.zeros(bs, 1, device=dev)
        rule = dict(codec.codec_rule(model, "content"), finished=done)
        rec = torch.zeros(bs, 4, dtype=torch.int32, device=dev)
        err = torch.zeros(bs, dtype=torch.int32, device=dev)
        tg = torch.randint(0, model.content_pad_code, (bs,), device=dev)
        words = torch.zeros(bs * 400, dtype=torch.int32, device=dev)
        state = torch.tensor([[1 << 40, 2, i * 400, 400] for i in range(bs)], dtype=torch.int64, device=dev)
        gen = torch.tensor([5, 0], dtype=torch.int64, device=dev)

        def decode():
            state[:, 1] = 2                                  # (keeps the cursor inside the stream; one small launch of its own)
            K.codec_decode_step(lg, state, words, err, **rule)

        for name, fn in (("dvq_codec_record", lambda: K.codec_record(lg, tg, rec, 1, err, **rule)),
                         ("dvq_codec_decode_step (+ cursor reset)", decode),
                         ("dvq_sample_constrained (top_k 300) + counter", lambda: K.sample_constrained(lg, 1.0, state=gen, top_k=300,
                                                                                                        sample=True, **rule))):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            t0 = time.perf_counter()
            ev[0].record()
            for _ in range(300):
                fn()
            ev[1].record()
            host = (time.perf_counter() - t0) / 300 * 1e6
            torch.cuda.synchronize()
            lines.append(f"  batch {bs:3d}  {name:46s} {ev[0].elapsed_time(ev[1]) / 300 * 1e3:7.1f} / {host:7.1f}")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
