"""Drop-in for the reference's evaluate.py: same flags, model-path expansion
(comma list or glob), linear ensemble average, metrics, printed lines and
CSV; inference runs on libjr (MI355X).

  python evaluate.py (-e | -m | -o --data_dir D) [-lm PATHS] [-so CSV] [-b 32] [-op 0.5]
Multi-GPU: torchrun --nproc-per-node N evaluate.py ... shards whole batches
(dataset order, so every BN batch is the reference's, App. C Q1) across
ranks with no collective on the data path; rank 0 gathers the [N] per-model
predictions, averages and scores them.

The reference restores and runs one member at a time, re-reading and
re-decoding the test set per member (evaluate.py:166-211).  Here every
member is resident on the GPU at once (one engine each: parameters plus
batch-32 buffers, a few GB per member against 288 GB of HBM), and each test
batch is decoded once and run through all members -- the same batches, so
the same batch-statistics BN (App. C Q1) and the same predictions.

Not in the reference: --bn moving (frozen BN; --x6h_frozen keeps the x6h
arithmetic there, guarded on the GPU), --tta, and --attribution
{gradient,integrated} --attribution_dir DIR, which under --bn moving also
writes per-image saliency maps of the logit (jr.attribution): DIR/maps_<k>.npy
per test batch k (float32 [n, h, w], the mean over members) and DIR/index.csv
(batch,row,label,prediction); stdout and the CSV stay byte-equal.
"""
import argparse
import csv
import os
import random
import sys
from glob import glob

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lib.dataset  # noqa: E402
import lib.metrics  # noqa: E402

# evaluate.py:24-29
DEFAULT_EYEPACS_DIR = "./data/eyepacs/bin2/test"
DEFAULT_MESSIDOR_DIR = "./data/messidor/bin2"
DEFAULT_LOAD_MODEL_PATH = "./tmp/model"
DEFAULT_SAVE_OPERATING_THRESHOLDS_PATH = "./tmp/test_op_pts.csv"
DEFAULT_BATCH_SIZE = 32

# evaluate.py:96-101
NUM_CHANNELS = 3
NUM_WORKERS = 8
NUM_THRESHOLDS = 200
KEPSILON = 1e-7


class _Parser(argparse.ArgumentParser):
    """The flag combinations that are refused, at parse time (no GPU involved)."""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if a.attribution is not None:
            if a.bn != "moving":
                self.error("--attribution requires --bn moving: only under frozen BN statistics is the gradient of "
                           "an image's logit a property of that image (with batch statistics it leaks into the batch)")
            if a.tta != "none":
                self.error("--attribution refuses --tta other than none: a map belongs to one view of the image")
            if a.attribution_dir is None:
                self.error("--attribution requires --attribution_dir DIR")
            if a.attribution_steps < 1:
                self.error("--attribution_steps must be at least 1")
        if a.x6h_frozen:
            if a.bn != "moving":
                self.error("--x6h_frozen requires --bn moving: it is the guarded frozen-BN forward of x6h (with batch "
                           "statistics x6h needs no guard)")
            if a.dtype != "f32":
                self.error("--x6h_frozen requires --dtype f32: x6h is an fp32 convolution arithmetic")
            if a.conv_math != "x6h":
                self.error("--x6h_frozen requires --conv_math x6h (the default)")
        return a


def build_parser():
    p = _Parser(
        description="Evaluate performance of trained graph on test data set. "
                    "Specify --data_dir if you use the -o param.")
    p.add_argument("-m", "--messidor", action="store_true", help="evaluate performance on Messidor-Original")
    p.add_argument("-e", "--eyepacs", action="store_true", help="evaluate performance on EyePacs set")
    p.add_argument("-o", "--other", action="store_true", help="evaluate performance on your own dataset")
    p.add_argument("--data_dir", help="directory where data set resides")
    p.add_argument("-lm", "--load_model_path", default=DEFAULT_LOAD_MODEL_PATH,
                   help="path to where graph model should be loaded from creates an ensemble if paths are "
                        "comma separated or a regexp")
    p.add_argument("-so", "--save_operating_thresholds_path", default=DEFAULT_SAVE_OPERATING_THRESHOLDS_PATH,
                   help="path to where operating points metrics should be saved")
    p.add_argument("-b", "--batch_size", default=DEFAULT_BATCH_SIZE, help="batch size")
    p.add_argument("-op", "--operating_threshold", default=0.5, help="operating threshold")
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"],
                   help="activation storage and conv arithmetic: f32 (the reference's; default) or bf16 MFMA")
    p.add_argument("--conv_math", default="x6h", choices=["x8", "x8p", "x6h", "f32"],
                   help="fp32 convolution arithmetic: x6h = power-of-two-scaled 3-way fp16 split, six f16 MFMAs per "
                        "product (fp32-accurate, default: 8.5 %% faster than x8 on the 10-member ensemble, "
                        "profiles/r06_ab_ens_x8_x6h.txt), x8 = exact 3-way bf16 split, x8p = x8 on pre-split "
                        "operand planes, f32 = fp32 MFMA")
    p.add_argument("--per_member", action="store_true",
                   help="one engine per ensemble member (default: every member's layers in one grouped launch, "
                        "jr.ensemble; predictions are bitwise the same)")
    # batch-independent inference (not in the reference, whose BN always uses batch statistics)
    p.add_argument("--bn", default="batch", choices=["batch", "moving"],
                   help="BN statistics: batch (the reference's: every prediction depends on its evaluation batch; "
                        "default) or moving (the moving averages saved by train.py --bn_moving, frozen: an image's "
                        "prediction depends on that image alone)")
    p.add_argument("--bn_calibrate_dir", default=None, metavar="DIR",
                   help="with --bn moving: instead of saved statistics, average the batch statistics of the first "
                        "--bn_calibrate_batches batches of the tfrecords in DIR (for checkpoints trained without "
                        "--bn_moving; in memory, nothing is written)")
    p.add_argument("--bn_calibrate_batches", type=int, default=16, metavar="K")
    p.add_argument("--x6h_frozen", action="store_true",
                   help="with --bn moving, --dtype f32 and --conv_math x6h: keep x6h under the frozen statistics "
                        "instead of falling back to x8.  The activation scale stays the engine's constant bound, and "
                        "every BN + ReLU output is checked against it on the GPU as it is stored: predictions are "
                        "bitwise independent of the other images of the batch, and an activation above the bound "
                        "stops the run with an error (repeat it without this flag) instead of saturating fp16.  The "
                        "x6h input gradient of --attribution scales each layer's gradient by its measured per-batch "
                        "maximum, so maps are batch-independent to within the x6h error class, not bitwise.  Measured "
                        "(profiles/frozen_x6h.txt, 299^2, batch 32): the grouped 10-member frozen forward is 4-7 %% "
                        "faster than on x8; one engine per member (--per_member, --attribution) is about 2x slower "
                        "on x6h than on x8, frozen or not")
    # the moving average of the weights (not in the reference; train.py --weight_ema)
    p.add_argument("--weights", default="trained", choices=["trained", "averaged"],
                   help="which weights of every checkpoint to evaluate: trained (the data file; default) or averaged "
                        "(the moving average train.py --weight_ema saved beside it as <path>.ema).  With --bn moving, "
                        "averaged needs --bn_calibrate_dir: the saved BN statistics belong to the trained weights")
    # test-time augmentation (not in the reference, which scores one view of every image)
    p.add_argument("--tta", default="none", choices=["none", "flips", "d4"],
                   help="average every member's prediction over views of each test batch, resampled on the GPU: "
                        "flips (4 views: the two mirrors and both) or d4 (8 views: the quarter turns, plain and "
                        "mirrored; square images); default none (one view, the reference's)")
    # per-image saliency maps (not in the reference)
    p.add_argument("--attribution", default=None, choices=["gradient", "integrated"],
                   help="with --bn moving: write per-image saliency maps of the logit (jr.attribution) -- gradient "
                        "(max over channels of |d logit / d pixel|) or integrated (integrated gradients from the "
                        "black image); one engine per member, the map is the mean over members")
    p.add_argument("--attribution_dir", default=None, metavar="DIR",
                   help="where --attribution writes maps_<batch>.npy (float32 [n, h, w]) and index.csv")
    p.add_argument("--attribution_steps", type=int, default=16, metavar="M",
                   help="integration steps of --attribution integrated (midpoint rule; default 16)")
    return p


def tta_views(tta, height, width):
    """The (flags, matrix) views of a --tta mode, in the order they are averaged (jr.augment)."""
    from jr import augment
    return {"flips": augment.flip_views, "d4": lambda: augment.d4_views(height, width)}[tta]()


def expand_model_paths(load_model_path: str):
    """evaluate.py:74-83: comma list, or glob when the path holds '*', '+'
    or '?' (each match's last extension stripped, duplicates removed).  Stems
    that are not complete checkpoints (a leftover `.data-*.tmp` of an
    interrupted save strips to `<path>.data-00000-of-00001`) are dropped."""
    from jr import checkpoint
    if "," in load_model_path:
        return load_model_path.split(",")
    if any(ch in load_model_path for ch in "*+?"):
        stems = {".".join(x.split(".")[:-1]) for x in glob("{}*".format(load_model_path))}
        return sorted(s for s in stems if checkpoint.exists(s))
    return [load_model_path]


def load_averaged(paths, graph):
    """Every member's averaged weights (<path>.ema, flat Keras layout);
    SystemExit naming the first member that has none."""
    from jr import checkpoint
    flats = []
    for path in paths:
        ema = checkpoint.load_ema(path, graph)
        if ema is None:
            raise SystemExit(f"{path}: checkpoint carries no averaged weights (trained without train.py "
                             "--weight_ema); --weights trained evaluates the weights it has")
        flats.append(ema[0])
    return flats


def make_engines(paths, meta, batch_size, device=0, conv_math="x6h", dtype="f32", grouped=False, input_grad=False,
                 x6h_frozen=False, flats=None):
    """The ensemble's inference engines, parameters loaded; conv tiles from
    the committed MI355X table of the eval workload (tiles="pinned"; the
    heuristic where none matches): every member and every run sums in the
    same order.  grouped: ONE jr.ensemble.EnsembleEngine holding every member
    (one launch per layer for all members); else one jr.Engine per member
    (input_grad: each with the buffers of Engine.input_gradient).
    x6h_frozen: the engines' guarded frozen forward on x6h (--x6h_frozen).
    flats: every member's parameters in place of its data file (--weights averaged)."""
    from jr import checkpoint
    from jr.engine import Engine
    if grouped and conv_math != "x8p":
        from jr.ensemble import EnsembleEngine
        params = flats if flats is not None else [checkpoint.load(path, None)[0] for path in paths]
        return EnsembleEngine(params, batch_size, meta["height"], meta["width"], meta.get("units", 1), device=device,
                              dtype=dtype, conv_math=conv_math if dtype == "f32" else "bf16", x6h_frozen=x6h_frozen)
    engines = []
    for k, path in enumerate(paths):
        eng = Engine(batch_size, meta["height"], meta["width"], meta.get("units", 1), device=device,
                     train=False, dtype=dtype, conv_math=conv_math if dtype == "f32" else "bf16",
                     input_grad=input_grad, x6h_frozen=x6h_frozen)
        flat = flats[k] if flats is not None else checkpoint.load(path, eng.g)[0]
        eng.load_params(flat)
        engines.append(eng)
    return engines


def load_bn_stats(paths, graph):
    """Every member's saved moving BN statistics and the meta entry of the
    first; SystemExit naming the first member that has none."""
    from jr import checkpoint
    stats = []
    for path in paths:
        st = checkpoint.load_bn_moving(path, graph)
        if st is None:
            raise SystemExit(f"{path}: checkpoint carries no moving BN statistics (trained without train.py "
                             "--bn_moving); --bn_calibrate_dir DIR computes them from the tfrecords in DIR")
        stats.append(st)
    return stats, checkpoint.read_meta(paths[0])["bn_moving"]


class Members:
    """The ensemble as predict_all and freeze_engines see it, whichever way it is held: a list of
    jr.Engine (one per member) or one jr.ensemble.EnsembleEngine (every member's layer in one launch).
    every: what set_batch / forward / freeze_bn are called on; count: the members; g: their graph;
    device: where they live; predictions(n): [M][n, 1] of the batch just run."""

    def __init__(self, engines):
        self.engines, self.grouped = engines, hasattr(engines, "members")
        self.every = [engines] if self.grouped else list(engines)
        self.count = engines.members if self.grouped else len(self.every)
        self.g, self.device = self.every[0].g, self.every[0].device

    def predictions(self, n):
        return list(self.engines.predictions(n)) if self.grouped else [e.predictions(n) for e in self.every]

    def upload(self, x):
        """One device copy of a uint8 batch for every member and view (it crosses PCIe once), waited for."""
        import torch
        xd = torch.as_tensor(x).to(self.device)
        torch.cuda.current_stream(self.device).synchronize()
        return xd

    def run(self, x, y, bn, **tables):
        """[M][n, 1]: one batch (a host array or upload()'s copy) through every member.  Every
        member's forward is enqueued before the first result is read back: one host sync per
        batch, not per member.  tables: set_batch's augment / warp of a test-time view."""
        n = 0
        for e in self.every:
            n = e.set_batch(x, y, **tables)
            e.forward(n, bn=bn)
        return self.predictions(n)


def _members(engines):
    return engines if isinstance(engines, Members) else Members(engines)


def freeze_engines(engines, stats=None, calibrate_dir=None, batches=16, batch_size=DEFAULT_BATCH_SIZE):
    """Frozen BN for every member: from saved statistics (one dict per
    member), or calibrated on the first `batches` batches of calibrate_dir
    (jr.Engine.calibrate_bn).  Returns the number of calibration batches."""
    mem = _members(engines)
    k = 0
    if calibrate_dir is not None:
        for e in mem.every:
            dataset = lib.dataset.initialize_dataset(
                calibrate_dir, batch_size, num_workers=NUM_WORKERS, prefetch_buffer_size=2 * batch_size,
                image_data_format="channels_last", num_channels=NUM_CHANNELS, image_dim=[mem.g.height, mem.g.width],
                decode_dtype="uint8", shard=(0, 1))
            it = iter(dataset)
            try:
                k = e.calibrate_bn(x for j, (x, _) in zip(range(batches), it))
            finally:
                lib.dataset.close_iterator(it)
    else:       # the grouped engine takes the list, a member's engine its own
        for e, st in zip(mem.every, [stats] if mem.grouped else stats):
            e.load_bn_moving(st)
    for e in mem.every:
        e.freeze_bn("moving")
    return k


def predict_views(engines, x, y, views, bn="batch"):
    """[M][n, 1]: every member's prediction of one uint8 batch, averaged over
    `views` ((flags, matrix) pairs of jr.augment) in their order.  The batch
    crosses PCIe once; each view re-runs the input kernel from the device
    copy (jr_image_u8_warp_augment_nhwc), then every member's forward."""
    from jr import augment
    mem = _members(engines)
    xd = mem.upload(x)
    seen = []       # [view][member][n, 1]
    for view in views:
        tab, warp = augment.view_tables(view, len(x))
        seen.append(mem.run(xd, y, bn, augment=tab, warp=warp))
    return [np.mean(np.array([v[m] for v in seen]), axis=0) for m in range(len(seen[0]))]


def member_mean(maps):
    """The fp32 mean of the members' maps, summed in member order."""
    s = np.asarray(maps[0], np.float32)
    for m in maps[1:]:
        s = s + np.asarray(m, np.float32)
    return s / np.float32(len(maps))


def write_maps(engines, n, k, attribution):
    """maps_<k>.npy of test batch k (its global index): the member mean of
    jr.attribution.attribute on the batch every engine holds."""
    from jr.attribution import attribute
    maps = [attribute(e, attribution["method"], attribution["steps"], B=n).cpu().numpy() for e in engines]
    os.makedirs(attribution["dir"], exist_ok=True)
    np.save(os.path.join(attribution["dir"], f"maps_{k:06d}.npy"), member_mean(maps))


def write_index(path, labels, predictions, batch_size):
    """index.csv: one line per test image in dataset order -- its batch (the
    k of maps_<k>.npy), its row there, its label and the ensemble prediction."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["batch", "row", "label", "prediction"])
        for i in range(len(labels)):
            w.writerow([i // batch_size, i % batch_size, int(labels[i, 0]), "{:.9g}".format(float(predictions[i, 0]))])


def predict_all(engines, data_dir, batch_size, rank=0, world=1, bn="batch", tta="none", attribution=None):
    """Per-member predictions over this rank's batches: ([M][n_r, 1], [n_r, 1],
    batch indices).  Each batch is decoded once (this rank's batches only)
    and run through every member, while the decoder threads already work on
    the next batches.  bn: "batch", or "frozen" (freeze_engines).
    tta: "none", or a mode of tta_views -- a member's prediction is then its
    mean over those views of the batch (predict_views).  attribution: None, or
    {"method", "steps", "dir"} -- after a batch's predictions are read, its
    saliency maps are written (write_maps; per-member engines, frozen BN)."""
    mem = _members(engines)
    dataset = lib.dataset.initialize_dataset(
        data_dir, batch_size, num_workers=NUM_WORKERS, prefetch_buffer_size=2 * batch_size,
        image_data_format="channels_last", num_channels=NUM_CHANNELS,
        image_dim=[mem.g.height, mem.g.width], decode_dtype="uint8",
        shard=(rank, world))
    preds = [[] for _ in range(mem.count)]
    views = None if tta == "none" else tta_views(tta, mem.g.height, mem.g.width)
    got_y, ids = [], []
    it = iter(dataset)
    try:
        for k, (x, y) in enumerate(it):
            ids.append(k * world + rank)
            got_y.append(y)
            if views is not None:
                batch = predict_views(mem, x, y, views, bn)
            else:       # the grouped engine stages the host array itself; members share one device copy
                batch = mem.run(x if mem.grouped else mem.upload(x), y, bn)
            for m, p in enumerate(batch):
                preds[m].append(p)
            if attribution is not None and views is None and not mem.grouped:
                write_maps(mem.every, len(batch[0]), ids[-1], attribution)
    finally:
        lib.dataset.close_iterator(it)
    empty = np.zeros((0, 1), np.float32)
    preds = [np.vstack(p) if p else empty for p in preds]
    labels = np.vstack(got_y) if got_y else empty
    return preds, labels, ids


def merge_ranks(gathered, batch_size, members):
    """(preds [M][n, 1], labels [n, 1]) in dataset order from every rank's (batch indices, preds,
    labels) of predict_all: each rank holds whole batches of batch_size, but for the last batch of
    the dataset, which may be partial, on the rank that got it; a rank may hold no batch at all."""
    pieces = []
    for o, p, y in gathered:
        sizes = np.cumsum([0] + [batch_size] * len(o))
        if len(o) and y.shape[0] < sizes[-1]:
            sizes[-1] = y.shape[0]
        for k, bi in enumerate(o):
            pieces.append((bi, [m[sizes[k]:sizes[k + 1]] for m in p], y[sizes[k]:sizes[k + 1]]))
    pieces.sort(key=lambda t: t[0])
    preds = [np.vstack([pc[1][m] for pc in pieces]) for m in range(members)]
    return preds, np.vstack([pc[2] for pc in pieces])


# ---- main()'s three parts
def choose_data_dir(parser, args):
    """The data directory of -e / -m / -o --data_dir; None (the refusal and the help are printed) where
    the flags name no single data set."""
    # evaluate.py:53-56 (chained comparison kept as is, App. C Q5)
    if bool(args.eyepacs) == bool(args.messidor) == bool(args.other):
        print("Can only evaluate one data set at once!")
    elif args.data_dir is not None:
        return str(args.data_dir)
    elif args.eyepacs:
        return DEFAULT_EYEPACS_DIR
    elif args.messidor:
        return DEFAULT_MESSIDOR_DIR
    else:
        print("Please specify --data_dir.")
    parser.print_help()
    return None


def build_members(args, paths, batch_size, r):
    """(engines, attribution): every member resident on device r.local with the weights (--weights)
    and the BN statistics (--bn) the flags name, frozen where they say so; rank 0 prints what was chosen."""
    from jr import checkpoint
    from jr.inception import build_inception_v3
    say = print if r.rank == 0 else (lambda *a, **k: None)
    meta = checkpoint.read_meta(paths[0])
    graph = lambda: build_inception_v3(meta["height"], meta["width"], meta.get("units", 1))  # noqa: E731
    # (before any engine is built: d4 refuses images that are not square)
    n_views = len(tta_views(args.tta, meta["height"], meta["width"])) if args.tta != "none" else 1
    conv_math, bn_stats, bn_info = args.conv_math, None, None
    flats = None
    if args.weights == "averaged":              # before any engine is built
        flats = load_averaged(paths, graph())
        say("Weights: averaged (the moving averages saved by train.py --weight_ema)")
    if args.bn == "moving":
        if args.bn_calibrate_dir is None:       # before any engine is built
            bn_stats, bn_info = load_bn_stats(paths, graph())
        if args.dtype == "f32" and conv_math == "x6h" and not args.x6h_frozen:
            conv_math = "x8"
            say("--bn moving: conv_math x8 is used instead of x6h (x6h scales activations by a bound that "
                "holds only for values standardised by their own batch's statistics)")
    attribution = None
    if args.attribution is not None:
        attribution = {"method": args.attribution, "steps": args.attribution_steps, "dir": str(args.attribution_dir)}
        # (stderr: stdout stays byte-equal to the run without --attribution)
        say(f"--attribution {args.attribution}: one engine per member (as --per_member), each with input-gradient "
            f"buffers; maps to {attribution['dir']}", file=sys.stderr)
    engines = make_engines(paths, meta, batch_size, device=r.local, conv_math=conv_math,
                           dtype=args.dtype, grouped=not (args.per_member or attribution),
                           input_grad=attribution is not None, x6h_frozen=args.x6h_frozen, flats=flats)
    if args.bn == "moving":
        k = freeze_engines(engines, bn_stats, args.bn_calibrate_dir, args.bn_calibrate_batches, batch_size)
        if bn_info is not None:
            say(f"BN statistics: moving (momentum {bn_info['momentum']}, {bn_info['updates']} updates)")
        else:
            say(f"BN statistics: moving (calibrated on {k} batches of {args.bn_calibrate_dir})")
    if args.tta != "none":
        say(f"Test-time augmentation: {args.tta} ({n_views} views)")
    return engines, attribution


def score(preds, labels, thresholds, save_path, attribution=None, batch_size=DEFAULT_BATCH_SIZE):
    """evaluate.py:214-250: the linear ensemble average, its Brier score, AUC, confusion matrix at the
    operating threshold (the last of `thresholds`), the printed lines and the operating-point CSV."""
    from jr import cli
    from jr.session import Session
    avg_pred = np.mean(np.array(preds), axis=0)          # evaluate.py:214-217
    if attribution is not None:
        write_index(os.path.join(attribution["dir"], "index.csv"), labels, avg_pred, batch_size)
    sess = Session(None, thresholds, NUM_THRESHOLDS, KEPSILON)
    sess.reset()
    sess.update(labels, avg_pred)
    spec, sens = sess.specificities(), sess.sensitivities()
    print(f"Brier score: {sess.value('brier'):6.4}, AUC: {sess.value('auc'):10.8}")
    print(f"Confusion matrix at operating threshold {thresholds[-1]:0.3f}")
    print(sess.confusion_matrix()[0])
    print("Specificity: {0:0.4f}, Sensitivity: {1:0.4f} at Operating Threshold {2:0.4f}.".format(
        spec[-1], sens[-1], thresholds[-1]))
    cli.write_operating_points(save_path, thresholds, spec, sens, NUM_THRESHOLDS)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    data_dir = choose_data_dir(parser, args)
    if data_dir is None:
        return 2
    if args.weights == "averaged" and args.bn == "moving" and args.bn_calibrate_dir is None:
        raise SystemExit("--weights averaged --bn moving needs --bn_calibrate_dir DIR: the BN statistics saved with a "
                         "checkpoint belong to its trained weights, not to the averaged ones")
    from jr import _ffi, cli

    load_model_paths = expand_model_paths(str(args.load_model_path))
    batch_size = int(args.batch_size)
    operating_threshold = float(args.operating_threshold)
    save_path = str(args.save_operating_thresholds_path)
    # (the only collective here is the final all_gather_object of the predictions)
    r = cli.ranks()
    random.seed(432)
    if r.rank == 0:       # one copy of the reference's header lines, whatever the rank count
        cli.print_versions()
        print("""
Evaluating: {},
Saving operating thresholds metrics at: {},
Using operating treshold: {},
""".format(data_dir, save_path, operating_threshold))
        print("Trying to load model(s):\n{}".format("\n".join(load_model_paths)))
    thresholds = lib.metrics.generate_thresholds(NUM_THRESHOLDS, KEPSILON) + [operating_threshold]
    engines, attribution = build_members(args, load_model_paths, batch_size, r)
    try:
        preds, labels, order = predict_all(engines, data_dir, batch_size, r.rank, r.world,
                                           bn="frozen" if args.bn == "moving" else "batch", tta=args.tta,
                                           attribution=attribution)
    except _ffi.JRError as e:
        if args.x6h_frozen and e.status == _ffi.JR_ERR_DEVICE:     # the guard; no retry on another path here
            print("--x6h_frozen: an activation exceeded the x6h bound under the frozen BN statistics; the "
                  "predictions are invalid -- repeat the run without --x6h_frozen (x8)", file=sys.stderr)
        raise
    if r.dist:   # gather every rank's batches to rank 0, restore dataset order
        gathered = [None] * r.world
        r.dist.all_gather_object(gathered, (order, preds, labels))
        if r.rank == 0:
            preds, labels = merge_ranks(gathered, batch_size, len(load_model_paths))
    if not r.dist or r.rank == 0:
        score(preds, labels, thresholds, save_path, attribution, batch_size)
    if r.dist:
        r.dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
