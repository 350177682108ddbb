#!/usr/bin/env python3
"""Write a checkpoint whose `state_dict` IS the averaged model of a checkpoint trained with `train.py --ema_decay`
(docs/design/20-weight-ema.md).  CPU only.  `global_step` and `epoch` are kept, optimizer and scheduler states dropped, and
`"ema_exported": {"decay", "num_updates"}` records where the weights came from.  The output loads everywhere a plain checkpoint does
-- a stage-2 YAML's `ckpt_path`, every script here without --use_ema, the reference's own loaders.

    python scripts/tools/export_ema.py --in last.ckpt --out last_ema.ckpt
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def export(ckpt):
    """-> the exported checkpoint dict; KeyError when `ckpt` has no averaged weights"""
    from dynamicvectorquantization_amd.evaluate import checkpoint_state_dict
    out = {"state_dict": checkpoint_state_dict(ckpt, use_ema=True)}
    for k in ("global_step", "epoch"):
        if k in ckpt:
            out[k] = ckpt[k]
    out["ema_exported"] = {"decay": float(ckpt["ema"]["decay"]), "num_updates": int(ckpt["ema"]["num_updates"])}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--in", dest="src", type=str, required=True, help="checkpoint with an \"ema\" key")
    ap.add_argument("--out", dest="dst", type=str, required=True)
    opt = ap.parse_args(argv)
    import torch
    ckpt = torch.load(opt.src, map_location="cpu")
    try:
        out = export(ckpt)
    except KeyError as e:
        print(f"export_ema.py: {opt.src}: {e.args[0]}", file=sys.stderr)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(opt.dst)), exist_ok=True)
    tmp = opt.dst + ".tmp"
    torch.save(out, tmp)
    os.replace(tmp, opt.dst)
    print(f"{opt.dst}: {len(ckpt['ema']['state_dict'])} averaged tensors of {len(out['state_dict'])}, "
          f"decay {out['ema_exported']['decay']}, {out['ema_exported']['num_updates']} updates")
    return 0


if __name__ == "__main__":
    sys.exit(main())
