"""Command line of the training and evaluation loops (the reference's ``xmcgan/main.py``):

    python -m xmcgan_image_generation_amd.main --config coco_xmc --workdir DIR --mode train|test [--set key=value ...]

``--config`` names a module with a ``get_config()``: a bare name is looked up in ``xmcgan_image_generation_amd.configs``, a dotted
name is imported as it is, a path ending in ``.py`` is loaded from that file; ``NAME:FUNCTION`` calls another function of the module
(``coco_xmc:get_test_config``).  ``--set`` overrides single fields; the value is read as a Python literal when it is one, as a
string otherwise.  Started by ``torch.distributed.run`` (``RANK`` in the environment) the process joins the group first, one rank
per GPU, as ``bench.py`` does; ``train`` then exchanges gradients over RCCL and rank 0 writes the files.
"""
from __future__ import annotations

import argparse
import ast
import importlib
import importlib.util
import logging
import os


def load_config(spec: str):
    name, _, func = spec.partition(":")
    if name.endswith(".py"):
        module_spec = importlib.util.spec_from_file_location("xmc_config_file", name)
        module = importlib.util.module_from_spec(module_spec)
        module_spec.loader.exec_module(module)
    else:
        module = importlib.import_module(name if "." in name else f"{__package__}.configs.{name}")
    return getattr(module, func or "get_config")()


def apply_overrides(config, assignments):
    for item in assignments or ():
        key, sep, text = item.partition("=")
        if not sep or not key:
            raise ValueError(f"--set takes key=value, got {item!r}")
        try:
            value = ast.literal_eval(text)
        except (ValueError, SyntaxError):
            value = text
        config[key] = value
    return config


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m xmcgan_image_generation_amd.main", description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="module path or name of the configuration (NAME[:FUNCTION])")
    ap.add_argument("--workdir", required=True, help="work unit directory: checkpoints, metrics.jsonl, images/")
    ap.add_argument("--mode", default="train", choices=["train", "test"])
    ap.add_argument("--set", dest="overrides", action="append", metavar="KEY=VALUE", default=[])
    ap.add_argument("--inception-ckpt", default=None, help="--mode test: the converted Inception-v3 weights (default: random)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend under torch.distributed.run")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    config = apply_overrides(load_config(args.config), args.overrides)

    import torch
    from . import train_utils
    joined = False
    if "RANK" in os.environ:
        import torch.distributed as dist
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local_rank)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)
        joined = True
    try:
        if args.mode == "train":
            train_utils.train(config, args.workdir)
        else:
            train_utils.test(config, args.workdir, inception_ckpt_path=args.inception_ckpt)
    finally:
        if joined:
            torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
