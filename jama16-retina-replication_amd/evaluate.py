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
import lib.evaluation  # noqa: E402
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


def freeze_engines(engines, stats=None, calibrate_dir=None, batches=16, batch_size=DEFAULT_BATCH_SIZE):
    """Frozen BN for every member: from saved statistics (one dict per
    member), or calibrated on the first `batches` batches of calibrate_dir
    (jr.Engine.calibrate_bn).  Returns the number of calibration batches."""
    grouped = hasattr(engines, "members")
    every = [engines] if grouped else engines
    k = 0
    if calibrate_dir is not None:
        g = every[0].g
        for e in every:
            dataset = lib.dataset.initialize_dataset(
                calibrate_dir, batch_size, num_workers=NUM_WORKERS, prefetch_buffer_size=2 * batch_size,
                image_data_format="channels_last", num_channels=NUM_CHANNELS, image_dim=[g.height, g.width],
                decode_dtype="uint8", shard=(0, 1))
            it = iter(dataset)
            try:
                k = e.calibrate_bn(x for j, (x, _) in zip(range(batches), it))
            finally:
                lib.dataset.close_iterator(it)
    elif grouped:
        engines.load_bn_moving(stats)
    else:
        for e, st in zip(engines, stats):
            e.load_bn_moving(st)
    for e in every:
        e.freeze_bn("moving")
    return k


def predict_views(engines, x, y, views, bn="batch"):
    """[M][n, 1]: every member's prediction of one uint8 batch, averaged over
    `views` ((flags, matrix) pairs of jr.augment) in their order.  The batch
    crosses PCIe once; each view re-runs the input kernel from the device
    copy (jr_image_u8_warp_augment_nhwc), then every member's forward."""
    import torch
    from jr import augment
    grouped = hasattr(engines, "members")
    every = [engines] if grouped else engines
    xd = torch.as_tensor(x).to(every[0].device)
    torch.cuda.current_stream(every[0].device).synchronize()
    seen = []       # [view][member][n, 1]
    for view in views:
        tab, warp = augment.view_tables(view, len(x))
        n = 0
        for e in every:
            n = e.set_batch(xd, y, augment=tab, warp=warp)
            e.forward(n, bn=bn)
        seen.append(list(engines.predictions(n)) if grouped else [e.predictions(n) for e in every])
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
    and run through every member.  bn: "batch", or "frozen" (freeze_engines).
    tta: "none", or a mode of tta_views -- a member's prediction is then its
    mean over those views of the batch (predict_views).  attribution: None, or
    {"method", "steps", "dir"} -- after a batch's predictions are read, its
    saliency maps are written (write_maps; per-member engines, frozen BN)."""
    import torch
    grouped = hasattr(engines, "members")      # jr.ensemble.EnsembleEngine
    g = engines.g if grouped else engines[0].g
    dataset = lib.dataset.initialize_dataset(
        data_dir, batch_size, num_workers=NUM_WORKERS, prefetch_buffer_size=2 * batch_size,
        image_data_format="channels_last", num_channels=NUM_CHANNELS,
        image_dim=[g.height, g.width], decode_dtype="uint8",
        shard=(rank, world))
    preds = [[] for _ in range(engines.members if grouped else len(engines))]
    views = None if tta == "none" else tta_views(tta, g.height, g.width)
    got_y, ids = [], []
    it = iter(dataset)
    try:
        for k, (x, y) in enumerate(it):
            ids.append(k * world + rank)
            got_y.append(y)
            if views is not None:
                for m, p in enumerate(predict_views(engines, x, y, views, bn)):
                    preds[m].append(p)
                continue
            # every member's forward is enqueued before the first result is
            # read back (one host sync per batch, not per member), while the
            # decoder threads already work on the next batches
            if grouped:       # every member's layer in one launch
                n = engines.set_batch(x, y)
                engines.forward(n, bn=bn)
                for m, p in enumerate(engines.predictions(n)):
                    preds[m].append(p)
                continue
            # (the uint8 batch crosses PCIe once for all members)
            xd = torch.as_tensor(x).to(engines[0].device)
            torch.cuda.current_stream(engines[0].device).synchronize()
            n = 0
            for e in engines:
                n = e.set_batch(xd, y)
                e.forward(n, bn=bn)
            for m, e in enumerate(engines):
                preds[m].append(e.predictions(n))
            if attribution is not None:
                write_maps(engines, n, ids[-1], attribution)
    finally:
        lib.dataset.close_iterator(it)
    empty = np.zeros((0, 1), np.float32)
    preds = [np.vstack(p) if p else empty for p in preds]
    labels = np.vstack(got_y) if got_y else empty
    return preds, labels, ids


def _one_batch(x, y):
    """feed_dict_fn for lib.evaluation.perform_test: one batch, then the end
    of the pass (evaluate.py:114-118 feed_images)."""
    state = {"done": False}

    def feed():
        if state["done"]:
            raise StopIteration
        state["done"] = True
        return {"x": x, "y": y}
    return feed


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    # evaluate.py:53-56 (chained comparison kept as is, App. C Q5)
    if bool(args.eyepacs) == bool(args.messidor) == bool(args.other):
        print("Can only evaluate one data set at once!")
        parser.print_help()
        return 2
    if args.data_dir is not None:
        data_dir = str(args.data_dir)
    elif args.eyepacs:
        data_dir = DEFAULT_EYEPACS_DIR
    elif args.messidor:
        data_dir = DEFAULT_MESSIDOR_DIR
    else:
        print("Please specify --data_dir.")
        parser.print_help()
        return 2

    if args.weights == "averaged" and args.bn == "moving" and args.bn_calibrate_dir is None:
        raise SystemExit("--weights averaged --bn moving needs --bn_calibrate_dir DIR: the BN statistics saved with a "
                         "checkpoint belong to its trained weights, not to the averaged ones")

    import torch
    from jr import _ffi, checkpoint

    load_model_paths = expand_model_paths(str(args.load_model_path))
    batch_size = int(args.batch_size)
    operating_threshold = float(args.operating_threshold)
    save_path = str(args.save_operating_thresholds_path)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knobs for the N > 1 path on a one-GPU box (as bench.py's):
    # JR_ONE_DEVICE=1 puts every rank on cuda:0, JR_DIST_BACKEND=gloo replaces
    # RCCL (which refuses two ranks on one device); the only collective here
    # is the final all_gather_object of the predictions
    if os.environ.get("JR_ONE_DEVICE") == "1" or os.environ.get("JR_BENCH_ONE_DEVICE") == "1":
        local = 0
    backend = os.environ.get("JR_DIST_BACKEND", "nccl")
    dist = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    random.seed(432)
    if rank == 0:       # one copy of the reference's header lines, whatever the rank count
        print(f"Numpy version: {np.__version__}")
        print(f"Torch version: {torch.__version__} (libjr / MI355X backend)")
        print("""
Evaluating: {},
Saving operating thresholds metrics at: {},
Using operating treshold: {},
""".format(data_dir, save_path, operating_threshold))
        print("Trying to load model(s):\n{}".format("\n".join(load_model_paths)))

    thresholds = lib.metrics.generate_thresholds(NUM_THRESHOLDS, KEPSILON) + [operating_threshold]
    meta = checkpoint.read_meta(load_model_paths[0])
    # (before any engine is built: d4 refuses images that are not square)
    n_views = len(tta_views(args.tta, meta["height"], meta["width"])) if args.tta != "none" else 1
    conv_math, bn_stats, bn_info = args.conv_math, None, None
    flats = None
    if args.weights == "averaged":              # before any engine is built
        from jr.inception import build_inception_v3
        flats = load_averaged(load_model_paths, build_inception_v3(meta["height"], meta["width"], meta.get("units", 1)))
        if rank == 0:
            print("Weights: averaged (the moving averages saved by train.py --weight_ema)")
    if args.bn == "moving":
        if args.bn_calibrate_dir is None:       # before any engine is built
            from jr.inception import build_inception_v3
            bn_stats, bn_info = load_bn_stats(load_model_paths, build_inception_v3(
                meta["height"], meta["width"], meta.get("units", 1)))
        if args.dtype == "f32" and conv_math == "x6h" and not args.x6h_frozen:
            conv_math = "x8"
            if rank == 0:
                print("--bn moving: conv_math x8 is used instead of x6h (x6h scales activations by a bound that "
                      "holds only for values standardised by their own batch's statistics)")
    attribution = None
    if args.attribution is not None:
        attribution = {"method": args.attribution, "steps": args.attribution_steps, "dir": str(args.attribution_dir)}
        if rank == 0:       # (stderr: stdout stays byte-equal to the run without --attribution)
            print(f"--attribution {args.attribution}: one engine per member (as --per_member), each with input-gradient "
                  f"buffers; maps to {attribution['dir']}", file=sys.stderr)
    engines = make_engines(load_model_paths, meta, batch_size, device=local, conv_math=conv_math,
                           dtype=args.dtype, grouped=not (args.per_member or attribution),
                           input_grad=attribution is not None, x6h_frozen=args.x6h_frozen, flats=flats)
    if args.bn == "moving":
        k = freeze_engines(engines, bn_stats, args.bn_calibrate_dir, args.bn_calibrate_batches, batch_size)
        if rank == 0 and bn_info is not None:
            print(f"BN statistics: moving (momentum {bn_info['momentum']}, {bn_info['updates']} updates)")
        elif rank == 0:
            print(f"BN statistics: moving (calibrated on {k} batches of {args.bn_calibrate_dir})")
    if args.tta != "none" and rank == 0:
        print(f"Test-time augmentation: {args.tta} ({n_views} views)")
    try:
        preds, labels, order = predict_all(engines, data_dir, batch_size, rank, world,
                                           bn="frozen" if args.bn == "moving" else "batch", tta=args.tta,
                                           attribution=attribution)
    except _ffi.JRError as e:
        if args.x6h_frozen and e.status == _ffi.JR_ERR_DEVICE:     # the guard; no retry on another path here
            print("--x6h_frozen: an activation exceeded the x6h bound under the frozen BN statistics; the "
                  "predictions are invalid -- repeat the run without --x6h_frozen (x8)", file=sys.stderr)
        raise

    if dist:   # gather every rank's batches to rank 0, restore dataset order
        gathered = [None] * world
        dist.all_gather_object(gathered, (order, preds, labels))
        if rank != 0:
            dist.destroy_process_group()
            return 0
        pieces = []
        for o, p, y in gathered:
            sizes = np.cumsum([0] + [batch_size] * len(o))
            # the last batch may be partial
            if len(o) and y.shape[0] < sizes[-1]:
                sizes[-1] = y.shape[0]
            for k, bi in enumerate(o):
                pieces.append((bi, [m[sizes[k]:sizes[k + 1]] for m in p], y[sizes[k]:sizes[k + 1]]))
        pieces.sort(key=lambda t: t[0])
        preds = [np.vstack([pc[1][m] for pc in pieces]) for m in range(len(load_model_paths))]
        labels = np.vstack([pc[2] for pc in pieces])

    all_predictions = np.array(preds)
    avg_pred = np.mean(all_predictions, axis=0)          # evaluate.py:214-217
    all_y = labels
    if attribution is not None:
        write_index(os.path.join(attribution["dir"], "index.csv"), all_y, avg_pred, batch_size)

    names = {"tp": lib.metrics.true_positives_at_thresholds, "fp": lib.metrics.false_positives_at_thresholds,
             "fn": lib.metrics.false_negatives_at_thresholds, "tn": lib.metrics.true_negatives_at_thresholds}
    state = {k: lib.metrics.create_reset_metric(f, scope=k, thresholds=thresholds) for k, f in names.items()}
    state["brier"] = lib.metrics.create_reset_metric(lib.metrics.mean_squared_error, scope="brier")
    state["auc"] = lib.metrics.create_reset_metric(lib.metrics.auc, scope="auc")
    for value, update, reset in state.values():
        reset()
        update(all_y, avg_pred)
    tp, fp, fn, tn = (state[k][0]() for k in ("tp", "fp", "fn", "tn"))
    test_conf_matrix = lib.metrics.confusion_matrix(tp[-1], fp[-1], fn[-1], tn[-1])
    test_brier, test_auc = state["brier"][0](), state["auc"][0]()
    test_specificities = tn / (tn + fp + np.float32(KEPSILON))
    test_sensitivities = tp / (tp + fn + np.float32(KEPSILON))

    print(f"Brier score: {test_brier:6.4}, AUC: {test_auc:10.8}")
    print(f"Confusion matrix at operating threshold {operating_threshold:0.3f}")
    print(test_conf_matrix[0])
    print("Specificity: {0:0.4f}, Sensitivity: {1:0.4f} at Operating Threshold {2:0.4f}.".format(
        test_specificities[-1], test_sensitivities[-1], thresholds[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
    with open(save_path, "w") as f:
        w = csv.writer(f, delimiter=" ")
        w.writerow(["threshold", "specificity", "sensitivity"])
        for idx in range(NUM_THRESHOLDS):
            w.writerow(["{:0.4f}".format(v) for v in (thresholds[idx], test_specificities[idx],
                                                       test_sensitivities[idx])])
    if dist:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
