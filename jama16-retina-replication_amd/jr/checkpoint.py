"""Checkpoints in place of tf.train.Saver (train.py:207,267,273-274;
evaluate.py:174-175).

A checkpoint at `path` is three files, so the ensemble glob of
evaluate.py:78-85 (".".join(name.split(".")[:-1]) over glob(path*), deduped)
recovers `path` exactly as it does for TF's `.meta/.index/.data-*` trio:
  <path>.meta                   JSON: graph config (resolution, units, op
                                order) and the parameter table
  <path>.index                  JSON: name -> (shape, offset, size), sha256
  <path>.data-00000-of-00001    raw little-endian float32, the flat
                                parameter buffer (jr.init.param_layout)
Loading executes nothing from the files (JSON + raw floats only).

A checkpoint saved with moving BN statistics (train.py --bn_moving) has a
fourth file, and its .meta a "bn_moving" entry (momentum, updates, channels
per layer, sha256 of the file); checkpoints without them are unchanged:
  <path>.bnstats                raw little-endian float32: per conv2d_bn layer
                                in graph order, moving_mean[c] then
                                moving_variance[c]

A checkpoint saved with averaged weights (train.py --weight_ema) has a file
more, and its .meta a "weight_ema" entry (decay, warm flag, update count,
sha256 of the file); the data file still holds the trained weights:
  <path>.ema                    raw little-endian float32, the moving average
                                of the parameters in the data file's layout
"""
from __future__ import annotations

import hashlib
import json
import os
from typing import Optional, Tuple

import numpy as np

from .init import param_layout

DATA_SUFFIX = ".data-00000-of-00001"
BN_SUFFIX = ".bnstats"
EMA_SUFFIX = ".ema"
FORMAT = "jr-checkpoint-v1"


def _bn_names(graph):
    return [(f"batch_normalization_{n.idx + 1}/moving_mean", f"batch_normalization_{n.idx + 1}/moving_variance",
             n.cout) for n in graph.convs]


def save(path: str, graph, flat: np.ndarray, extra: dict | None = None, bn_moving: dict | None = None,
         weight_ema: dict | None = None) -> None:
    """bn_moving: None, or {"stats": {Keras name: values} (Engine.bn_moving_numpy),
    "momentum": float, "updates": int} -- written as <path>.bnstats.
    weight_ema: None, or {"flat": the averaged parameters (Engine.ema_numpy),
    "decay": float, "warm": bool, "updates": int} -- written as <path>.ema."""
    layout, total = param_layout(graph.params)
    flat = np.ascontiguousarray(flat, dtype="<f4")
    if flat.size != total:
        raise ValueError(f"flat parameter vector has {flat.size} values, layout needs {total}")
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    raw = flat.tobytes()
    meta = {"format": FORMAT, "height": graph.height, "width": graph.width, "units": graph.units,
            "model": "inception_v3", "num_params": graph.num_params(), **(extra or {})}
    bn_raw = None
    if bn_moving is not None:
        parts = []
        for mean, var, c in _bn_names(graph):
            for key in (mean, var):
                v = np.ascontiguousarray(bn_moving["stats"][key], dtype="<f4").reshape(-1)
                if v.size != c:
                    raise ValueError(f"{key}: {v.size} values, the layer has {c} channels")
                parts.append(v)
        bn_raw = np.concatenate(parts).tobytes()
        meta["bn_moving"] = {"momentum": float(bn_moving["momentum"]), "updates": int(bn_moving["updates"]),
                             "channels": [c for _, _, c in _bn_names(graph)],
                             "sha256": hashlib.sha256(bn_raw).hexdigest()}
    ema_raw = None
    if weight_ema is not None:
        ema = np.ascontiguousarray(weight_ema["flat"], dtype="<f4").reshape(-1)
        if ema.size != total:
            raise ValueError(f"averaged parameter vector has {ema.size} values, layout needs {total}")
        ema_raw = ema.tobytes()
        meta["weight_ema"] = {"decay": float(weight_ema["decay"]), "warm": bool(weight_ema["warm"]),
                              "updates": int(weight_ema["updates"]), "sha256": hashlib.sha256(ema_raw).hexdigest()}
    index = {"format": FORMAT, "total": total, "sha256": hashlib.sha256(raw).hexdigest(),
             "tensors": [{"name": n, "shape": list(s), "offset": o, "size": z} for n, s, o, z in layout]}
    tmp = path + DATA_SUFFIX + ".tmp"
    with open(tmp, "wb") as f:
        f.write(raw)
    os.replace(tmp, path + DATA_SUFFIX)
    if bn_raw is not None:
        with open(path + BN_SUFFIX + ".tmp", "wb") as f:
            f.write(bn_raw)
        os.replace(path + BN_SUFFIX + ".tmp", path + BN_SUFFIX)
    elif os.path.exists(path + BN_SUFFIX):      # statistics of a checkpoint this one replaces
        os.remove(path + BN_SUFFIX)
    if ema_raw is not None:
        with open(path + EMA_SUFFIX + ".tmp", "wb") as f:
            f.write(ema_raw)
        os.replace(path + EMA_SUFFIX + ".tmp", path + EMA_SUFFIX)
    elif os.path.exists(path + EMA_SUFFIX):     # the average of a checkpoint this one replaces
        os.remove(path + EMA_SUFFIX)
    with open(path + ".index", "w") as f:
        json.dump(index, f)
    with open(path + ".meta", "w") as f:
        json.dump(meta, f, indent=1)


def load(path: str, graph=None, verify: bool = True) -> Tuple[np.ndarray, dict]:
    """(flat float32 parameters, meta dict).  With `graph`, the tensor table
    must match its parameter layout exactly."""
    with open(path + ".meta") as f:
        meta = json.load(f)
    with open(path + ".index") as f:
        index = json.load(f)
    if meta.get("format") != FORMAT or index.get("format") != FORMAT:
        raise ValueError(f"{path}: not a {FORMAT} checkpoint")
    raw = open(path + DATA_SUFFIX, "rb").read()
    if verify and hashlib.sha256(raw).hexdigest() != index["sha256"]:
        raise ValueError(f"{path}: data checksum mismatch")
    flat = np.frombuffer(raw, dtype="<f4").astype(np.float32)
    if flat.size != index["total"]:
        raise ValueError(f"{path}: data size mismatch")
    if graph is not None:
        layout, total = param_layout(graph.params)
        want = [(n, list(s), o, z) for n, s, o, z in layout]
        got = [(t["name"], t["shape"], t["offset"], t["size"]) for t in index["tensors"]]
        if want != got or total != index["total"]:
            raise ValueError(f"{path}: parameter table does not match the model graph")
    return flat, meta


def read_meta(path: str) -> dict:
    """The graph configuration of a checkpoint, from <path>.meta only (no
    parameter read or checksum): what evaluate.py needs to size its engines."""
    with open(path + ".meta") as f:
        meta = json.load(f)
    if meta.get("format") != FORMAT:
        raise ValueError(f"{path}: not a {FORMAT} checkpoint")
    return meta


def exists(path: str) -> bool:
    return all(os.path.exists(path + s) for s in (".meta", ".index", DATA_SUFFIX))


def load_bn_moving(path: str, graph) -> Optional[dict]:
    """The moving BN statistics of a checkpoint by Keras name
    (Engine.load_bn_moving), or None when it carries none (saved without
    train.py --bn_moving, or before they existed).  A size or checksum
    mismatch of <path>.bnstats raises."""
    info = read_meta(path).get("bn_moving")
    if info is None:
        return None
    names = _bn_names(graph)
    if list(info.get("channels", [])) != [c for _, _, c in names]:
        raise ValueError(f"{path}: BN statistics do not match the model graph")
    if not os.path.exists(path + BN_SUFFIX):
        raise ValueError(f"{path}: .meta names BN statistics but {path + BN_SUFFIX} is missing")
    raw = open(path + BN_SUFFIX, "rb").read()
    if len(raw) != 8 * sum(c for _, _, c in names):
        raise ValueError(f"{path}: BN statistics size mismatch")
    if hashlib.sha256(raw).hexdigest() != info["sha256"]:
        raise ValueError(f"{path}: BN statistics checksum mismatch")
    flat = np.frombuffer(raw, dtype="<f4").astype(np.float32)
    out, off = {}, 0
    for mean, var, c in names:
        out[mean], out[var] = flat[off:off + c].copy(), flat[off + c:off + 2 * c].copy()
        off += 2 * c
    return out


def load_ema(path: str, graph) -> Optional[Tuple[np.ndarray, dict]]:
    """(flat float32 averaged parameters, the .meta "weight_ema" entry) of a
    checkpoint (Engine.load_ema, or Engine.load_params to run on them), or None
    when it carries none (saved without train.py --weight_ema).  A size or
    checksum mismatch of <path>.ema raises."""
    info = read_meta(path).get("weight_ema")
    if info is None:
        return None
    if not os.path.exists(path + EMA_SUFFIX):
        raise ValueError(f"{path}: .meta names averaged weights but {path + EMA_SUFFIX} is missing")
    raw = open(path + EMA_SUFFIX, "rb").read()
    _, total = param_layout(graph.params)
    if len(raw) != 4 * total:
        raise ValueError(f"{path}: averaged weights size mismatch")
    if hashlib.sha256(raw).hexdigest() != info["sha256"]:
        raise ValueError(f"{path}: averaged weights checksum mismatch")
    return np.frombuffer(raw, dtype="<f4").astype(np.float32), dict(info)
