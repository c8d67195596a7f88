"""Drop-in for the reference's train.py: same flags, constants, printed lines,
checkpoints and operating-point CSV; the graph/session machinery is replaced
by jr (libjr HIP kernels on MI355X).

  python train.py [-t TRAIN_DIR] [-v VAL_DIR] [-sm SAVE_MODEL_PATH]
                  [-ss SAVE_SUMMARIES_DIR] [-so SAVE_OPERATING_THRESHOLDS_PATH]
                  [-sgd]
Multi-GPU (data parallel, RCCL): torchrun --nproc-per-node N train.py ...
Reference behaviour kept: BN uses batch statistics in
training and validation (Q1); weights start from Keras default init (Q2);
images are channels_last (Q3: the reference's channels_first path is a
reshape that scrambles pixels, so it is not reproduced).
"""
import argparse
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lib.dataset  # noqa: E402
import lib.evaluation  # noqa: E402
import lib.metrics  # noqa: E402

# train.py:19-24
DEFAULT_TRAIN_DIR = "./data/eyepacs/bin2/train"
DEFAULT_VAL_DIR = "./data/eyepacs/bin2/validation"
DEFAULT_SAVE_MODEL_PATH = "./tmp/model"
DEFAULT_SAVE_SUMMARIES_DIR = "./tmp/logs"
DEFAULT_SAVE_OPERATING_THRESHOLDS_PATH = "./tmp/op_pts.csv"

# train.py:66-89
NUM_CHANNELS = 3
NUM_WORKERS = 8
LEARNING_RATE = 3e-3
MOMENTUM = 0.9
USE_NESTEROV = True
TRAIN_BATCH_SIZE = 64
NUM_EPOCHS = 200
WAIT_EPOCHS = 10
MIN_DELTA_AUC = 0.01
VAL_BATCH_SIZE = 64
NUM_THRESHOLDS = 200
KEPSILON = 1e-7
SHUFFLE_BUFFER_SIZE = 2048


GEOMETRY_FLAGS = ("augment_rotate", "augment_zoom", "augment_shift")


class _Parser(argparse.ArgumentParser):
    """The geometric augmentation flags are refinements of --augment: one of them without it is an error."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        given = [f for f in GEOMETRY_FLAGS if getattr(ns, f) is not None]
        if given and not ns.augment:
            self.error("--{} needs --augment".format(given[0]))
        if ns.optimizer is not None and ns.vanilla_sgd:
            self.error("--optimizer and -sgd both name the optimizer: give one of them")
        if ns.rmsprop is not None and ns.optimizer != "rmsprop":
            self.error("--rmsprop needs --optimizer rmsprop")
        if ns.weight_ema_no_warm and ns.weight_ema is None:
            self.error("--weight_ema_no_warm needs --weight_ema")
        if ns.dropout_seed is not None and ns.dropout is None:
            self.error("--dropout_seed needs --dropout")
        return ns


# ---- argparse types: a whole number from a bound, a finite float under a test, and the comma lists
def _int_arg(lo, what):
    """The type of a whole number >= lo, refused as 'expected <what>, got ...'."""
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"expected {what}, got {text!r}")
        if v < lo:
            raise argparse.ArgumentTypeError(f"expected {what}, got {text!r}")
        return v
    return parse


def _float_arg(text, ok, what):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected {what}, got {text!r}")
    if not (np.isfinite(v) and ok(v)):
        raise argparse.ArgumentTypeError(f"expected {what}, got {text!r}")
    return v


def _positive_float(text):
    return _float_arg(text, lambda v: v > 0, "a finite value > 0")


def _nonnegative_float(text):
    return _float_arg(text, lambda v: v >= 0, "a finite value >= 0")


def _unit_arg(what):
    """The type of a float in [0, 1)."""
    return lambda text: _float_arg(text, lambda v: 0.0 <= v < 1.0, what)


# augmentation
def _range_arg(text):
    """'LO,HI' -> (lo, hi)."""
    try:
        lo, hi = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected LO,HI, got {text!r}")
    return lo, hi


# the optimizer recipe
def _decay_arg(text):
    """'RATE,EPOCHS' -> (rate, epochs): a rate > 0 and a whole number of epochs >= 1."""
    try:
        rate, epochs = text.split(",")
        rate, epochs = _positive_float(rate), int(epochs)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected RATE,EPOCHS, got {text!r}")
    if epochs < 1:
        raise argparse.ArgumentTypeError(f"expected RATE,EPOCHS with EPOCHS >= 1, got {text!r}")
    return rate, epochs


def _rmsprop_arg(text):
    """'RHO,MOMENTUM,EPS' -> (rho, momentum, eps): rho and momentum in [0, 1), eps > 0."""
    what = "RHO,MOMENTUM,EPS with RHO and MOMENTUM in [0, 1) and EPS > 0"
    try:
        rho, momentum, eps = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected {what}, got {text!r}")
    if not (0.0 <= rho < 1.0 and 0.0 <= momentum < 1.0 and eps > 0.0 and np.isfinite(eps)):
        raise argparse.ArgumentTypeError(f"expected {what}, got {text!r}")
    return rho, momentum, eps


def build_parser():
    p = _Parser(
        description="Trains and saves neural network for detection of diabetic retinopathy.")
    p.add_argument("-t", "--train_dir", default=DEFAULT_TRAIN_DIR,
                   help="path to folder that contains training tfrecords")
    p.add_argument("-v", "--val_dir", default=DEFAULT_VAL_DIR,
                   help="path to folder that contains validation tfrecords")
    p.add_argument("-sm", "--save_model_path", default=DEFAULT_SAVE_MODEL_PATH,
                   help="path to where graph model should be saved")
    p.add_argument("-ss", "--save_summaries_dir", default=DEFAULT_SAVE_SUMMARIES_DIR,
                   help="path to folder where summaries should be saved")
    p.add_argument("-so", "--save_operating_thresholds_path", default=DEFAULT_SAVE_OPERATING_THRESHOLDS_PATH,
                   help="path to where operating points should be saved")
    p.add_argument("-sgd", "--vanilla_sgd", action="store_true",
                   help="use vanilla stochastic gradient descent instead of "
                        "nesterov accelerated gradient descent")
    # extras (not in the reference): resolution, epochs, seeds, device
    p.add_argument("--image_size", type=int, default=299, help="input resolution (299; 587 high-res variant)")
    p.add_argument("--num_epochs", type=int, default=NUM_EPOCHS)
    p.add_argument("--seed", type=int, default=0, help="weight init seed (ensemble member index)")
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"],
                   help="activation storage and conv arithmetic: f32 (the reference's; default) or bf16 MFMA "
                        "(BASELINE configs 3 and 5; parameters, gradients, momentum and BN statistics stay fp32)")
    p.add_argument("--conv_math", default="x6h", choices=["x8", "x8p", "x6h", "f32"],
                   help="fp32 convolution arithmetic (--dtype f32): x6h = power-of-two-scaled 3-way fp16 split, six "
                        "products on the matrix cores (fp32-accurate, default), x8 = exact 3-way bf16 split, eight "
                        "products, x8p = x8 on pre-split operand planes, f32 = fp32 MFMA")
    p.add_argument("--replica_dump_dir", default=None,
                   help="(data parallel check) every rank writes its parameters after each epoch as "
                        "<dir>/params_e<epoch>_r<rank>.npy (Keras layout, fp32)")
    p.add_argument("--tiles", default="pinned", choices=["pinned", "heuristic", "autotune"],
                   help="conv tile configs: pinned (default; the committed MI355X table of this workload, "
                        "jr/tiles_mi355x.json, else the heuristic), heuristic (a function of the layer shapes only) "
                        "-- with either, two runs on any MI355X sum in the same order and train bitwise-equal -- or "
                        "autotune (timed on rank 0 at start, broadcast to every rank); the table in use is saved in "
                        "the checkpoint .meta")
    p.add_argument("--tile_table", default=None,
                   help="checkpoint path (or JSON file) whose saved tile table to reuse: reproduces that run's "
                        "summation order exactly")
    p.add_argument("--shuffle_seed", type=int, default=None)
    p.add_argument("--max_steps_per_epoch", type=int, default=None)
    # on-device training augmentation (jr.augment; not in the reference: off by default)
    p.add_argument("--augment", action="store_true",
                   help="augment every training batch on the GPU: random flips, hue, saturation, contrast and "
                        "brightness jitter, clamped to [0, 1] (validation and the final sweep are never augmented)")
    p.add_argument("--augment_seed", type=int, default=0,
                   help="seed of the augmentation draws (rank r draws from PCG64([seed, r]))")
    p.add_argument("--augment_hue", type=float, default=None, help="hue shift range +-H in turns (default 0.2)")
    p.add_argument("--augment_saturation", type=_range_arg, default=None, metavar="LO,HI",
                   help="saturation factor range (default 0.5,1.5)")
    p.add_argument("--augment_contrast", type=_range_arg, default=None, metavar="LO,HI",
                   help="contrast factor range (default 0.5,1.5)")
    p.add_argument("--augment_brightness", type=float, default=None,
                   help="brightness shift range +-B of the [0, 1] pixel range (default 0.125)")
    p.add_argument("--no_augment_flip", action="store_true", help="no random left-right / up-down flips")
    # geometric augmentation (with --augment; each off by default): a per-image rotation, zoom and shift,
    # resampled bilinearly on the GPU, pixels from outside the source black
    p.add_argument("--augment_rotate", type=float, default=None, metavar="DEG",
                   help="rotate every training image by a random angle in +-DEG degrees")
    p.add_argument("--augment_zoom", type=_range_arg, default=None, metavar="LO,HI",
                   help="magnify every training image by a random factor in LO,HI")
    p.add_argument("--augment_shift", type=float, default=None, metavar="FRAC",
                   help="shift every training image by random fractions in +-FRAC of its width and height")
    # moving averages of the BN statistics (not updated by the reference's graph: off by default)
    p.add_argument("--bn_moving", type=float, nargs="?", const=0.99, default=None, metavar="MOMENTUM",
                   help="keep Keras-style moving averages of the BN batch statistics (momentum 0.99 when given "
                        "bare) and save them beside every checkpoint (<path>.bnstats) for evaluate.py --bn moving; "
                        "training and validation still normalise with batch statistics.  Under torchrun every rank "
                        "keeps the averages of its own batches (they match its own BN); rank 0's are saved")
    # the optimizer recipe (not in the reference: off by default; jr.schedule, jr.h jr_opt_*)
    p.add_argument("--learning_rate", type=_positive_float, default=None, metavar="LR",
                   help="base learning rate (default {})".format(LEARNING_RATE))
    p.add_argument("--lr_decay", type=_decay_arg, default=None, metavar="RATE,EPOCHS",
                   help="exponential staircase: multiply the learning rate by RATE every EPOCHS epochs")
    p.add_argument("--lr_warmup", type=_int_arg(0, "a count >= 0"), default=None, metavar="STEPS",
                   help="linear warmup of the learning rate from LR/STEPS over the first STEPS steps")
    p.add_argument("--weight_decay", type=_nonnegative_float, default=None, metavar="WD",
                   help="L2 weight decay on the conv filters and the dense kernel (never BN betas or the bias)")
    p.add_argument("--clip_norm", type=_positive_float, default=None, metavar="C",
                   help="clip the global gradient norm (after the all-reduce) to C; a step whose norm is not "
                        "finite is skipped either way once any of --lr_decay, --lr_warmup, --weight_decay, "
                        "--clip_norm is given")
    # the rest of the published Inception-v3 recipe (not in the reference: off by default; jr.h jr_rmsprop_*, jr_ema_*)
    p.add_argument("--optimizer", default=None, choices=["nesterov", "sgd", "adam", "rmsprop"],
                   help="the optimizer (default: nesterov, or sgd with -sgd; not together with -sgd)")
    p.add_argument("--rmsprop", type=_rmsprop_arg, default=None, metavar="RHO,MOMENTUM,EPS",
                   help="RMSProp's decay, momentum and epsilon (default 0.9,0.9,1.0; with --optimizer rmsprop)")
    p.add_argument("--weight_ema", type=_unit_arg("a decay in [0, 1)"), nargs="?", const=0.9999, default=None,
                   metavar="DECAY",
                   help="keep a moving average of the weights (decay 0.9999 when given bare) on the GPU: validation, "
                        "early stopping and the final sweep then run on the averaged weights, and every checkpoint "
                        "carries both the trained weights and the average (<path>.ema, evaluate.py --weights averaged)")
    p.add_argument("--weight_ema_no_warm", action="store_true",
                   help="a fixed decay from the first step (default: min(DECAY, (1 + t) / (10 + t)) at update t)")
    # the loss recipe and dropout (not in the reference: off by default; jr.h jr_loss_spec, jr_dropout_*).  With any
    # of the first three the `Xent:` of the status line and the validation loss are the training objective
    # (smoothed, weighted, focal), no longer the plain cross-entropy
    p.add_argument("--label_smoothing", type=_unit_arg("a smoothing in [0, 1)"), default=None, metavar="E",
                   help="smooth the labels towards 1/2 by E in [0, 1) (0.1 in the published Inception-v3 recipe); "
                        "the `Xent:` status value is then the training objective")
    p.add_argument("--pos_weight", type=_positive_float, default=None, metavar="W",
                   help="weight the positive class's term of the loss by W > 0 (an imbalanced label); the `Xent:` "
                        "status value is then the training objective")
    p.add_argument("--focal_gamma", type=_nonnegative_float, default=None, metavar="G",
                   help="focal exponent G >= 0 on both terms of the loss; the `Xent:` status value is then the "
                        "training objective")
    p.add_argument("--dropout", type=_unit_arg("a rate in [0, 1)"), default=None, metavar="RATE",
                   help="drop the pooled features before the dense layer at RATE in [0, 1) in training steps only "
                        "(0.2 in the published Inception-v3 recipe); a new mask every step, drawn on the GPU")
    p.add_argument("--dropout_seed", type=int, default=None, metavar="N",
                   help="seed of the dropout masks (default 0; rank r draws stream r of it; with --dropout)")
    # gradient accumulation (not in the reference: off by default; jr.h jr_grad_accumulate)
    p.add_argument("--accum_steps", type=_int_arg(1, "a count >= 1"), default=None, metavar="K",
                   help="accumulate K batches of {0} per optimizer update ({0} * K images per GPU and update, every "
                        "batch under its own BN statistics; default 1): --lr_decay epochs, --lr_warmup and the "
                        "`Step:` of the status line then count updates, and a partial group at the end of an epoch "
                        "is closed there".format(TRAIN_BATCH_SIZE))
    p.add_argument("--status_every", type=_int_arg(1, "a whole number of batches >= 1"), default=1,
                   metavar="N",
                   help="print the status line every N batches (default 1: after every batch, which waits for "
                        "it).  N > 1 keeps the loss, the gradient norm and the Brier and threshold counts of "
                        "training, validation and the final sweep on the GPU, feeds batches through pinned "
                        "staging buffers and reads the step log once per N batches, so the GPU is not left idle "
                        "once per step; the end-of-epoch lines, summaries, checkpoints and the operating-point "
                        "CSV keep their meaning")
    return p


# ---- what each feature's flags mean: Engine keywords, checkpoint .meta entries, start-up lines
def augment_spec(args):
    """The jr.augment.AugmentSpec of the --augment* flags (None: --augment is off)."""
    if not args.augment:
        return None
    from jr.augment import AugmentSpec
    over = {"flip": not args.no_augment_flip}
    for key in ("hue", "saturation", "contrast", "brightness"):
        v = getattr(args, "augment_" + key)
        if v is not None:
            over[key] = v
    return AugmentSpec(**over)


def warp_spec(args):
    """The jr.augment.WarpSpec of the --augment_rotate / _zoom / _shift flags
    (None: none of them is given); an omitted one takes its identity value."""
    if not args.augment or all(getattr(args, f) is None for f in GEOMETRY_FLAGS):
        return None
    from jr.augment import WarpSpec
    return WarpSpec(rotate=args.augment_rotate or 0.0, zoom=args.augment_zoom or (1.0, 1.0),
                    shift=args.augment_shift or 0.0)


RECIPE_FLAGS = ("learning_rate", "lr_decay", "lr_warmup", "weight_decay", "clip_norm")


def opt_recipe(args):
    """The optimizer recipe of the flags as saved in the checkpoint .meta
    (None: none of them is given, the reference's settings)."""
    if all(getattr(args, f) is None for f in RECIPE_FLAGS):
        return None
    return {"learning_rate": LEARNING_RATE if args.learning_rate is None else args.learning_rate,
            "lr_decay": None if args.lr_decay is None else list(args.lr_decay),
            "lr_warmup": args.lr_warmup or 0, "weight_decay": args.weight_decay or 0.0, "clip_norm": args.clip_norm}


def opt_engine_kwargs(args):
    """Engine keywords of the recipe: the device optimizer path for every flag
    but a bare --learning_rate (none at all without a flag)."""
    if all(getattr(args, f) is None for f in RECIPE_FLAGS[1:]):
        return {}
    return {"weight_decay": args.weight_decay or 0.0, "clip_norm": args.clip_norm, "device_lr": True}


RMSPROP_DEFAULT = (0.9, 0.9, 1.0)


def optimizer_name(args):
    """The Engine's optimizer of the flags: --optimizer, else today's choice."""
    if args.optimizer is not None:
        return args.optimizer
    return "sgd" if args.vanilla_sgd else ("nesterov" if USE_NESTEROV else "momentum")


def optimizer_meta(args):
    """What --optimizer / --rmsprop / --weight_ema add to the recipe saved in the
    checkpoint .meta (nothing without them)."""
    out = {}
    if args.optimizer is not None:
        out["name"] = args.optimizer
        if args.optimizer == "rmsprop":
            out["rmsprop"] = dict(zip(("rho", "momentum", "epsilon"), args.rmsprop or RMSPROP_DEFAULT))
    if args.weight_ema is not None:
        out["weight_ema"] = {"decay": args.weight_ema, "warm": not args.weight_ema_no_warm}
    return out


def ema_engine_kwargs(args):
    """Engine keywords of --optimizer rmsprop and --weight_ema (none without them)."""
    kw = {}
    if args.optimizer == "rmsprop":
        kw.update(zip(("rmsprop_rho", "rmsprop_momentum", "rmsprop_eps"), args.rmsprop or RMSPROP_DEFAULT))
    if args.weight_ema is not None:
        kw.update(weight_ema=args.weight_ema, weight_ema_warm=not args.weight_ema_no_warm)
    return kw


LOSS_FLAGS = ("label_smoothing", "pos_weight", "focal_gamma", "dropout")


def loss_meta(args):
    """What --label_smoothing / --pos_weight / --focal_gamma / --dropout save as the
    "loss" entry of the checkpoint .meta (None: none of them is given)."""
    if all(getattr(args, f) is None for f in LOSS_FLAGS):
        return None
    return {"label_smoothing": args.label_smoothing or 0.0, "pos_weight": args.pos_weight,
            "focal_gamma": args.focal_gamma or 0.0, "dropout": args.dropout,
            "dropout_seed": (args.dropout_seed or 0) if args.dropout is not None else None}


def loss_engine_kwargs(args, rank=0):
    """Engine keywords of the loss and dropout flags (none without them); rank: the dropout stream."""
    kw = {}
    if args.label_smoothing is not None:
        kw["label_smoothing"] = args.label_smoothing
    if args.pos_weight is not None:
        kw["class_weight"] = [args.pos_weight]
    if args.focal_gamma is not None:
        kw["focal_gamma"] = args.focal_gamma
    if args.dropout is not None:
        kw.update(dropout=args.dropout, dropout_seed=args.dropout_seed or 0, dropout_stream=rank)
    return kw


def objective_line(args):
    """The start-up line that names the objective of the loss flags (None without them)."""
    m = loss_meta(args)
    if m is None:
        return None
    parts = ["sigmoid cross-entropy"]
    if m["label_smoothing"]:
        parts.append("label smoothing {:g}".format(m["label_smoothing"]))
    if m["pos_weight"] is not None:
        parts.append("positive weight {:g}".format(m["pos_weight"]))
    if m["focal_gamma"]:
        parts.append("focal gamma {:g}".format(m["focal_gamma"]))
    if m["dropout"] is not None:
        parts.append("dropout {:g} before the dense layer (seed {})".format(m["dropout"], m["dropout_seed"]))
    return "Objective: " + ", ".join(parts)


def accum_meta(args):
    """What --accum_steps adds to the checkpoint .meta and to the Engine's keywords (nothing without it)."""
    return {} if args.accum_steps is None else {"accum_steps": args.accum_steps}


def accum_line(args, world, batches):
    """The start-up line of --accum_steps (None without it); batches: per rank and epoch."""
    if args.accum_steps is None:
        return None
    from jr.schedule import accum_groups
    return ("Gradient accumulation: {0} batches of {1} per update, {2} images per update, {3} updates per epoch"
            .format(args.accum_steps, TRAIN_BATCH_SIZE, TRAIN_BATCH_SIZE * args.accum_steps * world,
                    accum_groups(batches, args.accum_steps)[1]))


def engine_kwargs(args, rank, local):
    """Every keyword the training Engine is built with: the reference's settings, then what each feature adds."""
    kw = {"device": local, "optimizer": optimizer_name(args),
          "lr": LEARNING_RATE if args.learning_rate is None else args.learning_rate, "momentum": MOMENTUM,
          "seed": args.seed, "dtype": args.dtype, "conv_math": args.conv_math if args.dtype == "f32" else "bf16",
          "tiles": "pinned" if args.tiles == "pinned" else "heuristic"}
    if args.bn_moving is not None:
        kw["bn_moving"] = args.bn_moving
    for more in (opt_engine_kwargs(args), ema_engine_kwargs(args), loss_engine_kwargs(args, rank), accum_meta(args)):
        kw.update(more)
    return kw


def run_meta(args, aug_spec, geo_spec):
    """What the run adds to every checkpoint's .meta beyond epoch, AUC and tile table:
    the augmentation, the optimizer and loss recipes, the accumulation and --status_every in use."""
    meta = {}
    if aug_spec:
        meta["augment"] = {"spec": aug_spec.to_meta(), "seed": args.augment_seed}
    if geo_spec:
        meta["augment_warp"] = {"spec": geo_spec.to_meta(), "seed": args.augment_seed}
    if opt_recipe(args) or optimizer_meta(args):
        meta["optimizer"] = {**(opt_recipe(args) or {}), **optimizer_meta(args)}
    if loss_meta(args):
        meta["loss"] = loss_meta(args)
    meta.update(accum_meta(args))
    if args.status_every > 1:
        meta["status_every"] = args.status_every
    return meta


def status_line(epoch, num_epochs, batch_num, xent, i_step=None):
    """train.py:191-203: one \\r-terminated status line."""
    width = len(str(num_epochs))
    parts = [f"Epoch: {epoch:>{width}}/{num_epochs:>{width}}", f"Batch: {batch_num:>4}, Xent: {xent:6.4}"]
    if i_step is not None:
        parts.append(f"Step: {i_step:>10}")
    return ", ".join(parts)


def load_tile_table(path: str) -> dict:
    """A saved tile table: from a checkpoint's .meta (jr.checkpoint) or a
    JSON file holding the table itself."""
    import json
    from jr import checkpoint
    if path.endswith(".json"):
        with open(path) as f:
            return json.load(f)
    meta = checkpoint.read_meta(path)
    if "tile_table" not in meta:
        raise ValueError(f"{path}: checkpoint carries no tile table")
    return meta["tile_table"]


# ---- the pieces of a run, in the order main() calls them
def open_datasets(args, r):
    """The training and validation sets.  Data parallel: every rank walks the same shuffled stream
    of record handles (rank 0's seed) and decodes only its own batches (b % world == rank);
    validation and the final sweep likewise, the metric counts summed over ranks (Session.end_pass)."""
    seed = args.shuffle_seed if args.shuffle_seed is not None else int.from_bytes(os.urandom(4), "little")
    if r.dist:
        import torch
        t = torch.tensor([seed], dtype=torch.int64, device=r.coll_dev)
        r.dist.broadcast(t, 0)
        seed = int(t.item())

    def dataset(path, batch, seed):
        return lib.dataset.initialize_dataset(
            path, batch, num_workers=NUM_WORKERS, prefetch_buffer_size=2 * TRAIN_BATCH_SIZE,
            shuffle_buffer_size=SHUFFLE_BUFFER_SIZE, image_data_format="channels_last", num_channels=NUM_CHANNELS,
            image_dim=[args.image_size, args.image_size], seed=seed, decode_dtype="uint8",
            shard=(r.rank, r.world) if r.dist else None)
    return dataset(args.train_dir, TRAIN_BATCH_SIZE, seed), dataset(args.val_dir, VAL_BATCH_SIZE, seed + 1)


def build_engine(args, r):
    """The Engine of the flags with its conv tile table: --tile_table's, or the one
    rank 0 timed under --tiles autotune (broadcast), else the engine's own."""
    from jr.engine import Engine
    engine = Engine(max(TRAIN_BATCH_SIZE, VAL_BATCH_SIZE), args.image_size, args.image_size,
                    **engine_kwargs(args, r.rank, r.local))
    table = None
    if args.tile_table:
        table = load_tile_table(args.tile_table)
    elif args.tiles == "autotune" and r.rank == 0:
        engine.autotune()
        table = engine.tile_table()
    if r.dist and args.tiles == "autotune" and not args.tile_table:
        box = [table]
        r.dist.broadcast_object_list(box, 0)
        table = box[0]
    if table is not None:
        engine.set_tile_table(table)
    return engine


def build_session(args, engine, thresholds, r):
    """The Session over the engine.  --status_every N > 1 is the loop that runs ahead of the host:
    the metrics stay on the device and the engine logs its steps, with room for N batches and the
    flush of a partial accumulation group.  Data parallel: the gradient exchange and the metric sum."""
    from jr.session import Session
    run_ahead = args.status_every > 1
    sess = Session(engine, thresholds, NUM_THRESHOLDS, KEPSILON, **({"device_metrics": True} if run_ahead else {}))
    sess.rank = r.rank
    if run_ahead:
        engine.step_log_enable(args.status_every + 1)
    if r.dist:
        import torch
        from jr.dist import BucketAllReduce
        sess.allreduce = BucketAllReduce(engine, r.world)

        def _sum_over_ranks(vec):
            t = torch.from_numpy(vec).to(r.coll_dev)
            r.dist.all_reduce(t)
            return t.cpu().numpy()
        sess.reduce = _sum_over_ranks
    return sess


class Augmenter:
    """One parameter table per training batch, each rank from its own stream.  The geometry
    draws from a generator of its own: the colour draws of a seed are the same with and without it."""

    def __init__(self, args, rank):
        self.spec, self.geo = augment_spec(args), warp_spec(args)
        self.size = (args.image_size, args.image_size)
        self.rng = np.random.Generator(np.random.PCG64([args.augment_seed, rank])) if self.spec else None
        self.geo_rng = np.random.Generator(np.random.PCG64([args.augment_seed, rank, 1])) if self.geo else None

    def draw(self, n):
        """Session.train_batch's (augment, warp) of a batch of n images; (None, None) without --augment."""
        if self.spec is None:
            return None, None
        from jr import augment
        warp = augment.draw_warp(self.geo, self.geo_rng, n, *self.size) if self.geo else None
        return augment.draw(self.spec, self.rng, n), warp


class Schedule:
    """The learning rate of every update on the device optimizer path (jr.schedule): the recipe's, its
    --lr_decay epochs counted in `epoch_updates` optimizer updates (every rank computes the same
    value from the same integers)."""

    def __init__(self, recipe, epoch_updates):
        self.base, self.warmup, self.decay = recipe["learning_rate"], recipe["lr_warmup"], None
        if recipe["lr_decay"]:
            self.decay = (recipe["lr_decay"][0], recipe["lr_decay"][1] * max(epoch_updates, 1))

    def rate(self, step) -> float:
        from jr.schedule import learning_rate
        return float(learning_rate(step, self.base, self.decay, self.warmup))


def plan_epoch(args, r, dataset):
    """(limit, sched).  limit: the batches of an epoch under data parallelism, where every rank runs the
    same number (matching collectives); else None.  sched: the Schedule of the device optimizer path,
    else None.  --accum_steps K: an update takes K batches (--max_steps_per_epoch still counts batches),
    ceil(batches / K) updates per epoch; its start-up line is printed here."""
    device_opt = bool(opt_engine_kwargs(args))
    if not (r.dist or device_opt or args.accum_steps is not None):
        return None, None       # (the records are counted only where the count is used)
    batches = -(-dataset.num_records() // TRAIN_BATCH_SIZE) // r.world
    limit = batches if r.dist else None
    if args.max_steps_per_epoch is not None:
        batches = min(batches, args.max_steps_per_epoch)
    sched = None
    if device_opt:
        from jr.schedule import accum_groups
        sched = Schedule(opt_recipe(args), accum_groups(batches, args.accum_steps or 1)[1])
    if r.rank == 0 and args.accum_steps is not None:
        print(accum_line(args, r.world, batches))
    return limit, sched


class UpdateTally:
    """The optimizer updates of one epoch on the device path: every update's gradient norm, how many
    the clip scaled and how many the non-finite guard skipped, and the last learning rate set."""

    def __init__(self, clip_norm=None):
        self.clip_norm, self.norms, self.clipped, self.skipped, self.step_lr = clip_norm, [], 0, 0, None

    def note(self, norm, skip) -> None:
        self.norms.append(norm)
        self.skipped += skip
        # (the kernel's own decision: fp32 norm against fp32 clip_norm)
        self.clipped += int(not skip and self.clip_norm is not None and np.float32(norm) > np.float32(self.clip_norm))

    def median(self) -> float:
        finite = [v for v in self.norms if np.isfinite(v)]      # (a skipped step's norm is inf or NaN)
        return float(np.median(np.asarray(finite, np.float64))) if finite else float("nan")

    def line(self) -> str:
        return ("Learning rate: {0:.6g}, median gradient norm: {1:.6g}, clipped steps: {2}, skipped steps: {3}"
                .format(self.step_lr, self.median(), self.clipped, self.skipped))

    def summary(self) -> dict:
        return {"grad_norm": self.median(), "learning_rate": self.step_lr}


def _look(engine, tally, run_ahead, device_opt, xent=None):
    """What the host learns when it looks at the device: the updates since its last look go to the
    tally, the newest batch's loss comes back.  Running ahead, both are in the step log (one
    synchronise for every batch since the last read); else they are the batch just run's own --
    `xent`, and engine.opt_step() (16 bytes, after a synchronise) when the batch closed an update."""
    if run_ahead:
        recs = engine.step_log_read()
        for rec in (recs[(recs["flags"] & 1) != 0] if device_opt else ()):
            tally.note(float(rec["grad_norm"]), int(rec["flags"]) >> 1 & 1)
        return float(recs["loss"][-1]) if len(recs) else None
    if device_opt and engine.accum_pending() == 0:
        norm, _, skip, _ = engine.opt_step()
        tally.note(norm, skip)
    return xent


def train_epoch(sess, engine, dataset, args, epoch, sched, aug, tally, rank, out=sys.stdout, limit=None):
    """The batches of one epoch.  Every --status_every-th batch the host looks (_look) and rank 0
    prints the status line; with N = 1 that is every batch, whose Brier sums are then added on the host.
    sched: the Schedule of the device optimizer path, else None; limit: plan_epoch's."""
    run_ahead, device_opt = args.status_every > 1, sched is not None
    sess.begin_pass("brier")
    batch_num = 0
    it = iter(dataset)
    try:
        for images, labels in it:
            if limit is not None and batch_num >= limit:
                break
            if args.max_steps_per_epoch is not None and batch_num >= args.max_steps_per_epoch:
                break
            if device_opt:
                tally.step_lr = sched.rate(sess.global_step)
                engine.set_lr(tally.step_lr)
            i_global, xent, probs = sess.train_batch(images, labels, *aug.draw(len(images)))
            if batch_num % args.status_every == args.status_every - 1:
                xent = _look(engine, tally, run_ahead, device_opt, xent)
                if rank == 0:
                    print(status_line(epoch, args.num_epochs, batch_num, xent, i_global), end="\r", file=out)
            if not run_ahead:       # (running ahead, train_batch left them on the device)
                sess.update(labels, probs, "brier")
            batch_num += 1
    finally:
        lib.dataset.close_iterator(it)
    # --accum_steps: a partial group is closed here, so validation, early stopping, checkpoints
    # and the replica check never see an open one (every rank ran the same number of batches)
    if sess.accum_flush() or run_ahead:
        _look(engine, tally, run_ahead, device_opt)
    sess.end_pass("brier")


def check_replicas(engine, args, epoch, r):
    """Data parallel: every rank applies the same update to the same
    reduced gradient, so the replicas must stay bitwise identical; compare
    a digest of every rank's parameters once per epoch (and dump them for
    --replica_dump_dir); with --weight_ema the digest covers the average too."""
    if not r.dist and not args.replica_dump_dir:
        return
    flat = engine.params_numpy()
    if args.replica_dump_dir:
        os.makedirs(args.replica_dump_dir, exist_ok=True)
        np.save(os.path.join(args.replica_dump_dir, f"params_e{epoch}_r{r.rank}.npy"), flat)
    if r.dist:
        import hashlib
        digest = hashlib.sha256(flat.tobytes())
        if args.weight_ema is not None:
            digest.update(engine.ema_numpy().tobytes())
        got = [None] * r.world
        r.dist.all_gather_object(got, digest.hexdigest())
        if len(set(got)) != 1:
            raise RuntimeError(f"data-parallel replicas diverged after epoch {epoch}: {got}")


def report_epoch(sess, tally, epoch, writer, out=sys.stdout):
    """Rank 0's lines at the end of an epoch's batches, and the summary of its updates."""
    print("\nEnd of epoch {0}! (Brier: {1:8.6})".format(epoch, sess.value("brier")), file=out)
    if tally.norms:
        print(tally.line(), file=out)
        writer.add_summary(tally.summary(), epoch)


class EarlyStop:
    """train.py:246-270: an epoch whose validation AUC does not beat the peak by MIN_DELTA_AUC
    waits; the run stops at such an epoch once WAIT_EPOCHS of them were waited (the test comes
    before the increment, as in the reference: WAIT_EPOCHS + 1 epochs without a new peak)."""
    min_delta, wait = MIN_DELTA_AUC, WAIT_EPOCHS

    def __init__(self):
        self.peak, self.waited = 0.0, 0

    def step(self, auc) -> str:
        """"peak" (a new one: save), "wait" or "stop"."""
        if auc < self.peak + self.min_delta:
            if self.wait == self.waited:
                return "stop"
            self.waited += 1
            return "wait"
        self.peak, self.waited = auc, 0
        return "peak"


def save_best(args, engine, epoch, val_auc, meta):
    """The checkpoint of a new peak: the weights, the run's .meta, and beside them the moving BN
    statistics (--bn_moving) and the weight average (--weight_ema)."""
    from jr import checkpoint
    extra = {}
    if args.bn_moving is not None:
        extra["bn_moving"] = {"stats": engine.bn_moving_numpy(), "momentum": args.bn_moving,
                              "updates": engine.updates}
    if args.weight_ema is not None:
        extra["weight_ema"] = {"flat": engine.ema_numpy(), "decay": args.weight_ema,
                               "warm": not args.weight_ema_no_warm, "updates": engine.ema_updates()}
    checkpoint.save(args.save_model_path, engine.g, engine.params_numpy(),
                    {"epoch": epoch, "val_auc": float(val_auc), "tile_table": engine.tile_table(), **meta}, **extra)


def restore_best(args, engine):
    """train.py:272-275: the best weights back into the engine, with the BN
    statistics and the average saved with them."""
    from jr import checkpoint
    flat, _ = checkpoint.load(args.save_model_path, engine.g)
    engine.load_params(flat)
    if args.bn_moving is not None:
        stats = checkpoint.load_bn_moving(args.save_model_path, engine.g)
        if stats is not None:
            engine.load_bn_moving(stats, checkpoint.read_meta(args.save_model_path)["bn_moving"]["updates"])
    if args.weight_ema is not None:
        ema = checkpoint.load_ema(args.save_model_path, engine.g)
        if ema is not None:
            engine.load_ema(ema[0], ema[1]["updates"])


def final_sweep(sess, dataset, averaged):
    """train.py:276-290: the threshold counts of the training set under the restored weights."""
    counts = ("tp", "fp", "fn", "tn")
    sess.begin_pass(*counts)
    it = iter(dataset)
    try:
        with averaged():
            for images, labels in it:
                sess.score_batch(images, labels, *counts)
    finally:
        lib.dataset.close_iterator(it)
    sess.end_pass(*counts)


BANNER = """
Training images folder: {0.train_dir},
Validation images folder: {0.val_dir},
Saving model and graph checkpoints at: {0.save_model_path},
Saving summaries at: {0.save_summaries_dir},
Saving operating points at: {0.save_operating_thresholds_path},
Use SGD: {1}
"""


def main(argv=None):
    args = build_parser().parse_args(argv)
    import contextlib
    from jr import cli
    from jr.summary import FileWriter

    random.seed(432)                       # train.py:17
    r = cli.ranks(versions_first=True)     # (rank 0: one copy of the reference's header lines)
    rank = r.rank
    if rank == 0:
        print(BANNER.format(args, bool(args.vanilla_sgd)))
    thresholds = lib.metrics.generate_thresholds(NUM_THRESHOLDS, KEPSILON) + [0.5]
    train_dataset, val_dataset = open_datasets(args, r)
    engine = build_engine(args, r)
    sess = build_session(args, engine, thresholds, r)
    aug = Augmenter(args, rank)
    meta = run_meta(args, aug.spec, aug.geo)
    if rank == 0 and loss_meta(args):
        print(objective_line(args))
    # --weight_ema: validation, early stopping and the final sweep read the averaged weights
    averaged = engine.averaged_weights if args.weight_ema is not None else contextlib.nullcontext
    writer = FileWriter(os.path.join(args.save_summaries_dir, "train")) if rank == 0 else None
    limit, sched = plan_epoch(args, r, train_dataset)

    stop, saved = EarlyStop(), False
    for epoch in range(args.num_epochs):
        tally = UpdateTally(args.clip_norm)
        train_epoch(sess, engine, train_dataset, args, epoch, sched, aug, tally, rank, limit=limit)
        check_replicas(engine, args, epoch, r)
        if rank == 0:
            report_epoch(sess, tally, epoch, writer)
        # every rank gets the same val_auc (summed counts), so the early-stop
        # decisions below agree and the collectives stay matched
        with averaged():
            val_auc = lib.evaluation.perform_test(sess=sess, init_op=val_dataset, summary_writer=writer, epoch=epoch)
        verdict = stop.step(val_auc)
        if verdict == "stop":
            if rank == 0:
                print("Stopped early at epoch {0} with saved peak auc {1:10.8}".format(epoch + 1, stop.peak))
            break
        if verdict == "peak":
            if rank == 0:
                print(f"New peak auc reached: {val_auc:10.8}")
                save_best(args, engine, epoch, val_auc, meta)
            saved = True

    # train.py:272-300: restore the best weights, sweep the training set,
    # write specificity/sensitivity per threshold.
    if r.dist:
        r.dist.barrier()
    if saved:
        restore_best(args, engine)
    final_sweep(sess, train_dataset, averaged)
    if rank == 0:
        cli.write_operating_points(args.save_operating_thresholds_path, thresholds,
                                   sess.specificities(), sess.sensitivities(), NUM_THRESHOLDS)
    if writer:
        writer.close()
    if r.dist:
        r.dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
