#!/usr/bin/env python3
"""`train.py` with the reference's command-line surface (train.py:27-50,58-270 of the reference) on the HIP
path, without pytorch_lightning / OmegaConf:

    python train.py --gpus -1 --base configs/stage1/dqvae-entropy-dual-r05_imagenet.yml --max_epochs 50 \
        model.params.lossconfig.params.perceptual_weight=0 model.params.lossconfig.params.disc_factor=0

* `-b/--base` YAMLs are merged left to right, then `key.sub=value` overrides (train.py:109-111);
* `--gpus N|-1|a,b,c`: one process per GPU; when launched under torchrun the env ranks are used, otherwise
  ranks are spawned here; gradients are averaged with RCCL (`trainer.GradBuckets`);
* learning rate = ngpu * batch_size * base_learning_rate (train.py:248-257);
* data: the BASELINE configs run on synthetic batches (`--synthetic`, default); a real
  `data:` section is instantiated only when its target is importable.
* `--gradient_clip_val X` (Lightning's Trainer flag): global-norm gradient clipping once per optimizer; `--skip_nonfinite_grads`:
  a step whose gradient holds an Inf / NaN leaves parameters and Adam moments untouched (docs/design/19-gradient-clipping.md).
* `--ema_decay D` (0: off): an exponential moving average of the weights of optimizer 0, used for validation and stored under the
  checkpoint's "ema" key; `--ema_no_warmup` drops the (1 + n) / (10 + n) warm-up of the decay (docs/design/20-weight-ema.md).
* `--deterministic` (Lightning's Trainer flag; off by default): every floating-point sum of the step in a fixed order and every host-side
  draw from the run's seed -- two runs with the same seed on one GPU walk the same trajectory bit for bit
  (docs/design/21-reproducible-training.md).  Stored in the run's saved config (`lightning.trainer.deterministic`), so `-r` keeps it.
* `-l/--logger none|csv|tensorboard` (or a comma list; default none) with `--log_every_n_steps N` (Lightning's flag, default 50): every
  scalar the model logs as `<key>_step` rows and `<key>_epoch` means in `<logdir>/metrics.csv` and / or a TensorBoard event file
  (docs/design/22-metrics-logging.md).  Stored in the saved config (`lightning.trainer.logger`, `.log_every_n_steps`), so `-r` keeps logging.
* `--track_grad_norm -1|2|inf` (Lightning's Trainer flag; -1 = off, the default) with `--track_norm_depth N` and `--no_track_updates`:
  per-parameter gradient, weight and update norms taken on the device, `<logdir>/norms.csv` and totals in the metrics row
  (docs/design/24-norm-tracking.md).  Stored in the saved config (`lightning.trainer.track_grad_norm`, ...), so `-r` keeps them.
Unsupported Trainer flags are accepted and ignored with a warning, like unknown Lightning flags would be.
"""
from __future__ import annotations

import argparse
import datetime
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("-n", "--name", type=str, const=True, default="", nargs="?", help="postfix for logdir")
    p.add_argument("-r", "--resume", type=str, const=True, default="", nargs="?", help="resume from logdir or checkpoint")
    p.add_argument("-b", "--base", nargs="*", metavar="base_config.yaml", default=list())
    p.add_argument("-s", "--seed", type=int, default=2021)
    p.add_argument("-f", "--postfix", type=str, default="")
    p.add_argument("-l", "--logger", type=str, default="none",
                   help="scalar logs of the run: none | csv (<logdir>/metrics.csv) | tensorboard (<logdir>/tensorboard/) | a comma list; "
                        "wandb is accepted and ignored")
    p.add_argument("--log_every_n_steps", type=int, default=50, help="with --logger: a row of `<key>_step` values every N steps (Lightning's Trainer flag)")
    p.add_argument("-d", "--debug", action="store_true")
    p.add_argument("-p", "--project", type=str, default="dvq")
    p.add_argument("--save_n", type=int, default=3, help="save top-n checkpoints by the model's `monitor` (train.py:48 of the reference)")
    p.add_argument("--check_val_every_n_epoch", type=int, default=1, help="validation pass every n epochs (0: never)")
    p.add_argument("--val_batches", type=int, default=4, help="synthetic data: batches per validation pass")
    p.add_argument("--activate_ddp_share", action="store_true")
    p.add_argument("--gpus", type=str, default="1")
    p.add_argument("--max_epochs", type=int, default=1)
    p.add_argument("--max_steps", type=int, default=-1)
    p.add_argument("--steps_per_epoch", type=int, default=100, help="synthetic data: batches per epoch")
    p.add_argument("--synthetic", action="store_true", default=True)
    p.add_argument("--real_data", action="store_true",
                   help="instantiate the config's `data:` section (data.build.DataModuleFromConfig -> GPU input pipeline, "
                        "$DVQ_IMAGENET_ROOT/train|val) instead of synthetic batches")
    p.add_argument("--device_jpeg", action="store_true",
                   help="with --real_data: JPEG files go through the device decoder (Huffman pass on host threads, inverse DCT, upsampling "
                        "and colour in HIP kernels; same pixels as PIL); other files are decoded by PIL as before")
    p.add_argument("--device_png", action="store_true",
                   help="with --real_data: PNG files are inflated on host threads and un-filtered in a HIP kernel (same pixels as PIL; "
                        "palette, 16-bit and interlaced files are decoded by PIL as before)")
    p.add_argument("--token_data", type=str, default="",
                   help="stage 2 only: train from this token set (scripts/tools/tokenize_dataset.py) instead of images -- no first-stage "
                        "forward, no image decoding")
    p.add_argument("--token_val", type=str, default="", help="with --token_data: the token set of the validation loop")
    p.add_argument("--precision", type=str, default="bf16", help="compute dtype of the HIP path: bf16 | fp32 | fp32x3 (fp32 tensors, products as three bf16 MFMA passes on split operands)")
    p.add_argument("--logdir", type=str, default="logs")
    p.add_argument("--save_every", type=int, default=0,
                   help="rewrite checkpoints/last.ckpt every N steps (0: once per epoch) -- atomic, rank 0 only")
    p.add_argument("--log_images_every", type=int, default=0,
                   help="write picture grids of the model's log_images every N batches to <logdir>/images/<split>/ (0: never; the "
                        "reference's CaptionImageLogger uses 50)")
    p.add_argument("--log_images_max", type=int, default=16, help="images per picture grid (4 per row)")
    p.add_argument("--gradient_clip_val", type=float, default=0.0,
                   help="clip the global gradient norm of each optimizer to this value (Lightning's Trainer flag; 0: off).  With -r the "
                        "value given on this command line applies: it is not stored in the saved configs")
    p.add_argument("--skip_nonfinite_grads", action="store_true",
                   help="skip the optimizer step (parameters and Adam moments untouched) when a gradient holds an Inf / NaN")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="decay of the weight EMA of optimizer 0 (autoencoder / transformer), e.g. 0.9999; 0: off.  Validation and the "
                        "monitored checkpoints then use the averaged weights, the checkpoint stores them under \"ema\".  With -r the "
                        "value given on this command line applies")
    p.add_argument("--ema_no_warmup", action="store_true",
                   help="use --ema_decay from the first update on, without the min(decay, (1 + n) / (10 + n)) warm-up")
    p.add_argument("--deterministic", action="store_true",
                   help="bit-reproducible training (Lightning's Trainer flag): ordered sums in every kernel of the step, host-side draws "
                        "seeded by --seed; slower.  One process on one GPU: with several ranks the collective's reduction order also counts")
    p.add_argument("--track_grad_norm", type=str, default="-1", choices=["-1", "2", "inf"],
                   help="per-parameter gradient, weight and update norms, taken on the device (Lightning's Trainer flag): -1 off, 2 or inf "
                        "choose what the total keys report.  <logdir>/norms.csv, rows at --log_every_n_steps")
    p.add_argument("--track_norm_depth", type=int, default=0,
                   help="with --track_grad_norm: one line per name prefix of N dotted components instead of one per parameter (0)")
    p.add_argument("--no_track_updates", action="store_true",
                   help="with --track_grad_norm: no update norms (saves the snapshot buffer, one copy of the parameters)")
    return p


def split_unknown(unknown):
    """arguments the parser did not take -> (`key.sub=value` config overrides, Trainer flags that are ignored with a warning)"""
    dot = [u for u in unknown if "=" in u and not u.startswith("--")]
    return dot, [u for u in unknown if u not in dot]


def _gpu_ids(spec: str, n_visible: int):
    """--gpus: "-1" = all visible devices, "N" = devices 0..N-1, "a,b,c" = exactly those device ids (train.py:61-62, Lightning)"""
    spec = spec.strip()
    if spec == "-1":
        return list(range(n_visible))
    if "," in spec:
        return [int(g) for g in spec.split(",") if g.strip() != ""]
    return list(range(int(spec)))


def run(rank, world, opt, unknown):
    import torch
    import torch.distributed as dist
    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.trainer import Trainer

    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world)
    if "LOCAL_RANK" in os.environ:                    # torchrun: the launcher's local rank is the device
        device_id = int(os.environ["LOCAL_RANK"])
    else:                                             # own spawn: rank r drives the r-th id of --gpus
        ids = _gpu_ids(opt.gpus, torch.cuda.device_count())
        device_id = ids[rank] if rank < len(ids) else rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(device_id)
    dev = torch.device("cuda", torch.cuda.current_device())
    rt.set_compute_dtype(opt.precision)
    torch.manual_seed(opt.seed)

    dot, ignored = split_unknown(unknown)
    if ignored and rank == 0:
        print(f"[train.py] ignoring unsupported Trainer flags: {ignored}")
    # -r <logdir | checkpoint>: continue IN that logdir with the configs it saved (train.py:73-89 of the reference), -b adds to them
    resume_ckpt, logdir = None, None
    if opt.resume:
        if os.path.isfile(opt.resume):
            resume_ckpt = opt.resume
            logdir = os.path.dirname(os.path.dirname(os.path.abspath(opt.resume)))
        else:
            logdir = opt.resume.rstrip("/")
            resume_ckpt = os.path.join(logdir, "checkpoints", "last.ckpt")
        saved_cfgs = sorted(os.path.join(logdir, "configs", f) for f in os.listdir(os.path.join(logdir, "configs"))) \
            if os.path.isdir(os.path.join(logdir, "configs")) else []
        opt.base = saved_cfgs + list(opt.base)
    if not opt.base:
        raise SystemExit("-b/--base <config.yaml> is required (or -r <logdir> holding configs/)")
    config = cfg.merge(*[cfg.load_yaml(b) for b in opt.base], cfg.from_dotlist(dot))
    # --deterministic lives in the saved config like the reference's lightning.trainer section: a resumed run keeps the mode it began in
    if opt.deterministic:
        config = cfg.merge(config, cfg.from_dotlist(["lightning.trainer.deterministic=true"]))
    deterministic = bool(config.get("lightning", {}).get("trainer", {}).get("deterministic", False))
    # -l/--logger and --log_every_n_steps likewise (docs/design/22-metrics-logging.md): a resumed run keeps writing the logs it began
    from dynamicvectorquantization_amd.metrics import parse_logger_flag
    writers, unsupported = parse_logger_flag(opt.logger)
    if unsupported and rank == 0:
        print(f"[train.py] ignoring unsupported loggers: {unsupported}")
    if writers:
        config = cfg.merge(config, {"lightning": {"trainer": {"logger": ",".join(writers), "log_every_n_steps": int(opt.log_every_n_steps)}}})
    saved_trainer = config.get("lightning", {}).get("trainer", {})
    writers, _ = parse_logger_flag(saved_trainer.get("logger", "none"))
    log_every_n_steps = int(saved_trainer.get("log_every_n_steps", opt.log_every_n_steps))
    # --track_grad_norm, --track_norm_depth, --no_track_updates likewise (docs/design/24-norm-tracking.md)
    if opt.track_grad_norm != "-1":
        config = cfg.merge(config, {"lightning": {"trainer": {"track_grad_norm": opt.track_grad_norm, "track_norm_depth": int(opt.track_norm_depth),
                                                              "track_updates": not opt.no_track_updates, "log_every_n_steps": int(opt.log_every_n_steps)}}})
        saved_trainer = config.get("lightning", {}).get("trainer", {})
    track_grad_norm = str(saved_trainer.get("track_grad_norm", "-1"))
    track_norm_depth = int(saved_trainer.get("track_norm_depth", 0))
    track_updates = bool(saved_trainer.get("track_updates", True))
    if logdir is None:
        now = datetime.datetime.now().strftime("%Y-%m-%dT%H-%M-%S")
        logdir = os.path.join(opt.logdir, now + ("_" + opt.name if opt.name else "") + opt.postfix)
    if world > 1:            # every rank must agree on the directory name (timestamps differ): rank 0's wins
        names = [logdir]
        dist.broadcast_object_list(names, src=0)
        logdir = names[0]
    ckpt_path = os.path.join(logdir, "checkpoints", "last.ckpt")
    if rank == 0 and not opt.resume:
        os.makedirs(os.path.join(logdir, "configs"), exist_ok=True)
        import yaml
        with open(os.path.join(logdir, "configs", "project.yaml"), "w") as f:
            yaml.safe_dump(cfg.to_plain(config), f)
    model = cfg.instantiate_from_config(config.model).to(dev)

    bs = config.data.params.batch_size
    model.steps_per_epoch = opt.steps_per_epoch
    model.training_steps = opt.steps_per_epoch * opt.max_epochs
    model.max_epoch = opt.max_epochs
    from dynamicvectorquantization_amd.trainer import reference_learning_rate
    model.learning_rate = reference_learning_rate(config.model, world, bs)
    if "base_learning_rate" in config.model and rank == 0:
        print("Setting learning rate to {:.2e} = {} (num_gpus) * {} (batchsize) * {:.2e} (base_lr)".format(
            model.learning_rate, world, bs, config.model.base_learning_rate))
    model.min_learning_rate = config.model.get("min_learning_rate", 0.)

    size = config.model.params.get("image_size", 256)
    real_iter = None
    if opt.real_data:
        # the YAML's own `data:` section through the plugin boundary: host threads decode, resize / crop / flip / normalise run
        # on the GPU (dynamicvectorquantization_amd/data.py); each rank shuffles with its own seed (weak scaling, bs per GPU).
        # Built BEFORE the Trainer: configure_optimizers() bakes steps_per_epoch / training_steps into the LR schedules
        config.data.params["device"] = str(dev)
        config.data.params["size"] = size
        if opt.device_jpeg:
            config.data.params["device_decode"] = True      # docs/design/23-device-jpeg.md
            if rank == 0:
                print("[train.py] device JPEG decode: Huffman pass on host threads, the rest on the GPU")
        if opt.device_png:
            config.data.params["device_png"] = True         # docs/design/29-device-png.md
            if rank == 0:
                print("[train.py] device PNG decode: inflate on host threads, un-filtering on the GPU")
        dm = cfg.instantiate_from_config(config.data)
        loader = dm.train_dataloader()
        loader.rng = __import__("numpy").random.default_rng(opt.seed + 977 * rank)
        opt.steps_per_epoch = model.steps_per_epoch = len(loader)
        model.training_steps = len(loader) * opt.max_epochs

        def _batches():
            while True:
                for b in loader:
                    yield {k: v for k, v in b.items() if torch.is_tensor(v)}      # strings (paths, synsets) stay on the host side
        real_iter = _batches()

    token_iter, token_vloader = None, None
    if opt.token_val and not opt.token_data:
        raise SystemExit("--token_val needs --token_data")
    if opt.token_data:
        # stored codes instead of images (docs/design/16-token-shards.md); like --real_data: built BEFORE the Trainer, one shuffle per rank
        if opt.real_data:
            raise SystemExit("--token_data and --real_data are two sources for the same batches: give one")
        if not hasattr(model, "forward_tokens"):
            raise SystemExit(f"--token_data trains a stage-2 (DQ-Transformer) model; {opt.base} builds {type(model).__name__}")
        from dynamicvectorquantization_amd import tokens as T

        def token_loader(path, shuffle, seed):
            ds = T.TokenShardDataset(path)
            ds.check_model(model)
            if len(ds) < bs:
                raise SystemExit(f"{path}: {len(ds)} images do not fill one batch of {bs}")
            return T.TokenBatchLoader(ds, bs, dev, model.permuter, shuffle=shuffle, seed=seed)
        tloader = token_loader(opt.token_data, True, opt.seed + 977 * rank)
        opt.steps_per_epoch = model.steps_per_epoch = len(tloader)
        model.training_steps = len(tloader) * opt.max_epochs
        if opt.token_val:
            token_vloader = token_loader(opt.token_val, False, opt.seed)

        def _token_batches():
            while True:
                for b in tloader:
                    yield b
        token_iter = _token_batches()

    total = model.training_steps if opt.max_steps < 0 else min(opt.max_steps, model.training_steps)
    metrics_logger = None
    if writers and rank == 0:            # rank 0 writes its own values, like Lightning does for keys logged without sync_dist
        from dynamicvectorquantization_amd.metrics import MetricsLogger
        metrics_logger = MetricsLogger(logdir, writers=writers, log_every_n_steps=log_every_n_steps)
    trainer = Trainer(model, max_steps=total, log_every=10 if rank == 0 else 0, gradient_clip_val=opt.gradient_clip_val,
                      skip_nonfinite=opt.skip_nonfinite_grads, ema_decay=opt.ema_decay, ema_warmup=not opt.ema_no_warmup,
                      deterministic=deterministic, metrics_logger=metrics_logger, track_grad_norm=track_grad_norm,
                      track_updates=track_updates, norm_every=log_every_n_steps, norm_depth=track_norm_depth,
                      norm_logdir=logdir if rank == 0 else None)
    pool = [torch.from_numpy(synth.half_flat_images(bs, size, seed=opt.seed + 977 * rank + i)).to(dev) for i in range(4)]

    image_key = getattr(model, "image_key", None) or getattr(model, "first_stage_key", "image")
    n_classes = None
    if getattr(model, "cond_stage_key", None) == "class_label":         # class-conditional stage 2: synthetic labels
        n_classes = int(getattr(model.cond_stage_model, "n_classes", 1000))

    def batch_fn(step):
        model.current_epoch = step // opt.steps_per_epoch
        if token_iter is not None:
            return next(token_iter)
        if real_iter is not None:
            b = next(real_iter)
            return {image_key: b["image"], **({"class_label": b["class_label"]} if "class_label" in b and n_classes is not None else {})}
        batch = {image_key: pool[step % len(pool)]}
        if n_classes is not None:
            g = torch.Generator().manual_seed(opt.seed + step)
            batch["class_label"] = torch.randint(0, n_classes, (bs,), generator=g).to(dev)
        return batch

    if resume_ckpt:
        trainer.load_state_dict(torch.load(resume_ckpt, map_location="cpu", weights_only=False))
        if rank == 0:
            print(f"resumed from {resume_ckpt} at global step {model.global_step}")
    # last.ckpt is rewritten (atomically, rank 0) every --save_every steps / once per epoch and at the end: a crashed or
    # preempted run continues with `-r <logdir>`
    # validation (Lightning's loop in the reference): the YAML's validation set with --real_data, else a fixed set of synthetic batches;
    # the model's `monitor` (val_rec_loss in the shipped stage-1 YAMLs) picks the --save_n best checkpoints kept beside last.ckpt
    val_fn = None
    if opt.check_val_every_n_epoch > 0 and hasattr(model, "validation_step"):
        if token_iter is not None:
            if token_vloader is not None:
                def val_fn():
                    return iter(token_vloader)
            elif rank == 0:
                print("no --token_val: training without the validation loop")
        elif opt.real_data and "validation" not in getattr(dm, "datasets", {"validation": None}):
            if rank == 0:
                print("the data config has no validation split: training without the validation loop")
        elif opt.real_data:
            vloader = dm.val_dataloader()

            def val_fn():
                for b in vloader:
                    yield {image_key: b["image"], **({"class_label": b["class_label"]} if "class_label" in b and n_classes is not None else {})}
        else:
            vpool = [torch.from_numpy(synth.half_flat_images(bs, size, seed=opt.seed + 7919 + 977 * rank + i)).to(dev)
                     for i in range(max(1, opt.val_batches))]

            def val_fn():
                for i, im in enumerate(vpool):
                    b = {image_key: im}
                    if n_classes is not None:
                        g = torch.Generator().manual_seed(opt.seed + 31 * i)
                        b["class_label"] = torch.randint(0, n_classes, (bs,), generator=g).to(dev)
                    yield b
    image_logger = None
    if opt.log_images_every > 0 and rank == 0:        # utils/logger.py:57-147 of the reference (train.py:214-221: every 50 batches, 16 images, clamp)
        from dynamicvectorquantization_amd.imagelog import ImageLogger
        image_logger = ImageLogger(logdir, batch_frequency=opt.log_images_every, max_images=opt.log_images_max, clamp=True, seed=opt.seed)
    trainer.fit(batch_fn, ckpt_path=ckpt_path, save_every=opt.save_every or opt.steps_per_epoch, is_rank0=rank == 0, val_fn=val_fn,
                val_every=opt.check_val_every_n_epoch * opt.steps_per_epoch, save_top_k=opt.save_n, image_logger=image_logger)
    if rank == 0:
        print("saved", ckpt_path)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    opt, unknown = get_parser().parse_known_args()
    if not opt.base and not opt.resume:
        raise SystemExit("-b/--base <config.yaml> is required")
    if opt.device_jpeg and not opt.real_data:
        raise SystemExit("--device_jpeg needs --real_data")
    if opt.device_png and not opt.real_data:
        raise SystemExit("--device_png needs --real_data")
    import torch
    if "WORLD_SIZE" in os.environ:          # launched by torchrun
        return run(int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), opt, unknown)
    ngpu = len(_gpu_ids(opt.gpus, torch.cuda.device_count()))
    if ngpu <= 1:
        return run(0, 1, opt, unknown)
    import torch.multiprocessing as mp
    mp.spawn(run, args=(ngpu, opt, unknown), nprocs=ngpu, join=True)


if __name__ == "__main__":
    main()
