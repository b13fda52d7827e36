"""RepVGG re-parameterisation — drop-in for wespeaker/models/convert_repvgg.py (the recipes' stage 4):
  --config C --load avg_model.pt --save convert_model.pt

Folds every block's branches (3x3, 1x1 or dilated 3x3, identity BatchNorm) of a training-form checkpoint
into one conv + bias (arch.repvgg_fold, float64 on the host; no device is touched), writes the deploy-form
state_dict (`rbr_reparam.*`, `seg.*`) to --save and rewrites the config with `model_args.deploy: true`, so
that what loads the pair builds the deploy layout.  The config goes to `<exp_dir>/config.yaml` when it
names an `exp_dir` (the recipes: the file --config already is), else back to --config.

Extraction gives the same embeddings either way: from avg_model.pt with the training config (the fold
then runs when the model goes to the device) or from convert_model.pt with the rewritten one."""
from __future__ import annotations

import argparse
import os

import torch
import yaml

from ..arch import make_spec, repvgg_fold, repvgg_params


def convert(config: str, load: str, save: str) -> str:
    """Returns the path of the config it wrote."""
    with open(config, "r", encoding="utf-8") as f:
        configs = yaml.safe_load(f)
    model_args = dict(configs.get("model_args") or {})
    model_args["deploy"] = False
    spec = make_spec(configs["model"], **model_args)
    if spec.family != "repvgg":
        raise ValueError(f"{configs['model']} is not a RepVGG model")
    state = torch.load(load, map_location="cpu", weights_only=True)
    for key in ("state_dict", "model"):  # checkpoint wrappers the reference tool unwraps
        if key in state:
            state = state[key]
            break
    state = {k.replace("module.", ""): v for k, v in state.items()}
    missing = [n for n, _ in repvgg_params(spec) if n not in state and not n.endswith("num_batches_tracked")]
    if missing:
        raise KeyError(f"{load}: not a training-form {spec.arch} checkpoint, missing {missing[:4]} ...")
    folded = repvgg_fold(spec, state)
    os.makedirs(os.path.dirname(os.path.abspath(save)), exist_ok=True)
    torch.save({k: torch.from_numpy(v) for k, v in folded.items()}, save)
    configs["model_args"] = dict(configs.get("model_args") or {}, deploy=True)
    out = os.path.join(configs["exp_dir"], "config.yaml") if configs.get("exp_dir") else config
    with open(out, "w", encoding="utf-8") as f:
        yaml.safe_dump(configs, f)
    print(f"==> Saving convert model to '{save}'")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="fold a training-form RepVGG checkpoint into its deploy form")
    ap.add_argument("--config", type=str, default="conf/config.yaml")
    ap.add_argument("--load", type=str, required=True)
    ap.add_argument("--save", type=str, required=True)
    a = ap.parse_args()
    convert(a.config, a.load, a.save)
