#!/usr/bin/env python3
"""Fixture train_entries.json: what the four trainers' entry points answer before their first HIP call -- the work-space
sizes over a table of configurations and the return code of every refusal.  tests/test_train_entries_cpu.py replays the
rows against the library of its own tree and expects the same integers; it imports the tables and the row runner from
here.

    python tests/golden/make_golden_train_entries.py [--package-root <built checkout>]

Reads this package alone (the built libonsetfp.so and _lib.py of the checkout named), no GPU and no reference.  A second
run writes the same bytes.

No row dereferences a device pointer: the entries check their arguments, the options and the work space's size on the
host, so a made-up non-NULL address stands for every buffer.

Contents:
  workspace[trainer]  rows [n, n_val, layers, norm, pool, options, stretch, older, older_random, grads], one per cell of
      batch {1, 5, 1024} x n_val {0, below n, above n} x layers {1, most} x (norm, pool) x options {none, dropout, source,
      source+span}: `stretch` is ofp_*_train_stretch_workspace_bytes; `older` the form without options (CNN, LCCCNN; it
      ignores them), `older_random` the form without a span and `grads` ofp_*_loss_grads_random_workspace_bytes (CNNRNN,
      RNN), both on rows without a span; null where the trainer has no such form.
  refusals  rows {trainer, entry, case, fields, cfg, n, n_val, options, patience, null, ws, rc}: `entry` is a public
      train, loss-and-gradients or work-space function, `fields` the configuration fields the case is about, `cfg` the
      changed fields (null: a NULL config), `null` the arguments passed as NULL, `ws` "short" for a work space one byte
      under the need and "none" for one of 0 bytes (what the other rows pass: their refusal comes earlier).  rc is the
      return code, -1 for a work-space function.
"""
import argparse
import ctypes
import importlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "train_entries.json"
FAKE = 0x1000  # stands for every device buffer
SPAN = 4
MAX_SHIFT = 2


def load_lib(root):
    root = str(Path(root).resolve())
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module("onset_fingerprinting_amd._lib")


# ---- the four trainers --------------------------------------------------------------------------------------------------
# base: a valid configuration; layers: (field, most); norm: the flag's field or None; stats: has a d_stats argument;
# train / grads / sizes: the public entries of each kind

def _cnn_base():
    return dict(n_conv=2, channels=[3, 4, 5, 6], kernel=3, padding=1, dilation=1, groups=1, act=1, batch_norm=1, pool=1,
                width=16, n_out=2, loss=0, bn_momentum=0.1, bn_eps=1e-5)


TRAINERS = {
    "cnn": dict(
        config="CnnConfig", base=_cnn_base(), layers=("n_conv", 3), norm="batch_norm", stats=True,
        train=["ofp_cnn_train", "ofp_cnn_train_random", "ofp_cnn_train_stretch"],
        grads=["ofp_cnn_loss_grads", "ofp_cnn_loss_grads_random"],
        older="ofp_cnn_train_workspace_bytes", older_random="ofp_cnn_train_random_workspace_bytes",
        stretch="ofp_cnn_train_stretch_workspace_bytes", grads_bytes=None, says="ofp_cnn"),
    "cccnn": dict(
        config="CccnnConfig",
        base=dict(n_conv=2, sensors=3, layer_sizes=[2] * 8, kernels=[3] * 8, strides=[1] * 8, padding=1, dilation=1,
                  group=0, act=1, norm=1, pool=1, width=256, n_out=2, loss=0, momentum=0.9, weight_decay=1e-4,
                  gn_eps=1e-5),
        layers=("n_conv", 8), norm="norm", stats=False,
        train=["ofp_cccnn_train", "ofp_cccnn_train_random", "ofp_cccnn_train_stretch"],
        grads=["ofp_cccnn_loss_grads", "ofp_cccnn_loss_grads_random"],
        older="ofp_cccnn_train_workspace_bytes", older_random="ofp_cccnn_train_random_workspace_bytes",
        stretch="ofp_cccnn_train_stretch_workspace_bytes", grads_bytes=None, says="ofp_cccnn"),
    "cnnrnn": dict(
        config="CnnrnnConfig", base=dict(cnn=_cnn_base(), hidden=8, heads=2), layers=("cnn.n_conv", 3),
        norm="cnn.batch_norm", stats=True, train=["ofp_cnnrnn_train_stretch"], grads=["ofp_cnnrnn_loss_grads_random"],
        older=None, older_random=None, stretch="ofp_cnnrnn_train_stretch_workspace_bytes",
        grads_bytes="ofp_cnnrnn_loss_grads_random_workspace_bytes", says="ofp_cnnrnn"),
    "rnn": dict(
        config="RnnConfig",
        base=dict(channels=3, width=12, hidden=8, layers=2, heads=2, n_out=2, loss=0, permute_input=1,
                  weight_decay=1e-4, ln_eps=1e-5),
        layers=("layers", 4), norm=None, stats=False, train=["ofp_rnn_train_stretch"],
        grads=["ofp_rnn_loss_grads_random"], older=None, older_random=None,
        stretch="ofp_rnn_train_stretch_workspace_bytes", grads_bytes="ofp_rnn_loss_grads_random_workspace_bytes",
        says="ofp_rnn"),
}

# Every configuration field just past its limit: (fields the case is about, changes to the base, options).  A flag has no
# limit of its own: its case is the refusal that only the flag brings about.
_CNN_LIMITS = [
    (["n_conv"], {"n_conv": 0}, "none"), (["n_conv"], {"n_conv": 4}, "none"),
    (["channels"], {"channels": [3, 129, 5, 6]}, "none"), (["channels"], {"channels": [0, 4, 5, 6]}, "none"),
    (["kernel"], {"kernel": 9}, "none"), (["kernel"], {"kernel": 0}, "none"),
    (["padding"], {"padding": -1}, "none"), (["padding"], {"padding": 513}, "none"),
    (["dilation"], {"dilation": 0}, "none"), (["dilation"], {"dilation": 65}, "none"),
    (["groups"], {"groups": 0}, "none"), (["groups"], {"groups": 2}, "none"),
    (["act"], {"act": -1}, "none"), (["act"], {"act": 6}, "none"),
    (["batch_norm"], {"width": 1, "kernel": 1, "padding": 0, "pool": 0, "n_conv": 1, "_n": 1}, "none"),
    (["pool"], {"width": 1, "kernel": 1, "padding": 0, "batch_norm": 0, "n_conv": 1}, "none"),
    (["width"], {"width": 513}, "none"), (["width"], {"width": 0}, "none"),
    (["n_out"], {"n_out": 17}, "none"), (["n_out"], {"n_out": 0}, "none"),
    (["loss"], {"loss": 2}, "none"), (["loss"], {"loss": -1}, "none"),
    (["bn_momentum", "batch_norm"], {"bn_momentum": 1.5}, "none"),
    (["bn_momentum", "batch_norm"], {"bn_momentum": 0.0}, "none"),
    (["bn_eps", "batch_norm"], {"bn_eps": 0.0}, "none"),
]

LIMITS = {
    "cnn": _CNN_LIMITS,
    "cnnrnn": [([f"cnn.{f}" for f in fields], {f"cnn.{k}" if not k.startswith("_") else k: v for k, v in ch.items()}, o)
               for fields, ch, o in _CNN_LIMITS] + [
        (["hidden"], {"hidden": 129}, "none"), (["hidden"], {"hidden": 0}, "none"),
        (["heads"], {"heads": 9, "hidden": 9}, "none"), (["heads"], {"heads": 0}, "none"),
        (["heads"], {"heads": 3}, "none"),
    ],
    "rnn": [
        (["channels"], {"channels": 9}, "none"), (["channels"], {"channels": 0}, "none"),
        (["width"], {"width": 513}, "none"), (["width"], {"width": 0}, "none"),
        (["hidden"], {"hidden": 129}, "none"), (["hidden"], {"hidden": 0}, "none"),
        (["layers"], {"layers": 5}, "none"), (["layers"], {"layers": 0}, "none"),
        (["heads"], {"heads": 9, "hidden": 9}, "none"), (["heads"], {"heads": 0}, "none"),
        (["heads"], {"heads": 3}, "none"),
        (["n_out"], {"n_out": 17}, "none"), (["n_out"], {"n_out": 0}, "none"),
        (["loss"], {"loss": 2}, "none"), (["loss"], {"loss": -1}, "none"),
        (["permute_input"], {"permute_input": 0}, "source"),
        (["weight_decay"], {"weight_decay": -1.0}, "none"),
        (["ln_eps"], {"ln_eps": 0.0}, "none"),
    ],
    "cccnn": [
        (["n_conv"], {"n_conv": 0}, "none"), (["n_conv"], {"n_conv": 9}, "none"),
        (["sensors"], {"sensors": 65}, "none"), (["sensors"], {"sensors": 0}, "none"),
        (["layer_sizes"], {"layer_sizes": [2, 65] + [2] * 6}, "none"),
        (["layer_sizes"], {"layer_sizes": [0] + [2] * 7}, "none"),
        (["kernels"], {"kernels": [65] + [3] * 7}, "none"), (["kernels"], {"kernels": [0] + [3] * 7}, "none"),
        (["strides"], {"strides": [5] + [1] * 7}, "none"), (["strides"], {"strides": [0] + [1] * 7}, "none"),
        (["padding"], {"padding": -1}, "none"), (["padding"], {"padding": 513}, "none"),
        (["dilation"], {"dilation": 0}, "none"), (["dilation"], {"dilation": 65}, "none"),
        (["group"], {"group": 1, "layer_sizes": [22] * 8}, "none"),
        (["act"], {"act": -1}, "none"), (["act"], {"act": 6}, "none"),
        (["norm", "gn_eps"], {"gn_eps": 0.0}, "none"),
        (["pool"], {"width": 1, "kernels": [1] * 8, "padding": 0, "n_conv": 1}, "none"),
        (["width"], {"width": 513}, "none"), (["width"], {"width": 0}, "none"),
        (["n_out"], {"n_out": 17}, "none"), (["n_out"], {"n_out": 0}, "none"),
        (["loss"], {"loss": 2}, "none"), (["loss"], {"loss": -1}, "none"),
        (["momentum"], {"momentum": 1.0}, "none"), (["momentum"], {"momentum": -0.5}, "none"),
        (["weight_decay"], {"weight_decay": -1.0}, "none"),
    ],
}

N, N_VAL = 5, 7  # the batch of the refusal rows


# ---- building the arguments ----------------------------------------------------------------------------------------------

def config_fields(L, trainer):
    """Dotted names of every field of the trainer's configuration."""
    def walk(cls, prefix):
        for name, typ in cls._fields_:
            if isinstance(typ, type) and issubclass(typ, ctypes.Structure):
                yield from walk(typ, prefix + name + ".")
            else:
                yield prefix + name
    return list(walk(getattr(L, TRAINERS[trainer]["config"]), ""))


def _fill(obj, values):
    for k, v in values.items():
        if isinstance(v, dict):
            _fill(getattr(obj, k), v)
        elif isinstance(v, list):
            arr = getattr(obj, k)
            for i, e in enumerate(v):
                arr[i] = e
        else:
            setattr(obj, k, v)


def make_config(L, trainer, changes):
    """The trainer's base configuration with `changes` (dotted field -> value; keys with '_' are not fields)."""
    cfg = getattr(L, TRAINERS[trainer]["config"])()
    _fill(cfg, TRAINERS[trainer]["base"])
    for k, v in changes.items():
        if k.startswith("_"):
            continue
        obj, path = cfg, k.split(".")
        for part in path[:-1]:
            obj = getattr(obj, part)
        _fill(obj, {path[-1]: v})
    return cfg


def window_of(cfg):
    """(channels, width) of the windows a configuration takes."""
    c = getattr(cfg, "cnn", cfg)
    if hasattr(c, "sensors"):
        return c.sensors, c.width
    ch = c.channels
    return (ch if isinstance(ch, int) else ch[0]), c.width


def make_random(L, cfg, n, options):
    """(ofp_train_random or None, stretch span) of `options`: none, dropout, source, source+span, span_one (a source
    and span 1), span_alone (a span and no options)."""
    if options == "none":
        return None, 0
    if options == "span_alone":
        return None, SPAN
    r = L.TrainRandom()
    r.seed = 3
    if options == "dropout":
        r.dropout_p = 0.5
        return r, 0
    span = {"source": 0, "source+span": SPAN, "span_one": 1}[options]
    channels, width = window_of(cfg) if cfg is not None else (1, 1)
    r.max_shift, r.n_extractions, r.n_onsets, r.audio_channels = MAX_SHIFT, 1, n, channels
    r.d_audio, r.d_starts, r.audio_len = FAKE, FAKE, width + 2 * MAX_SHIFT + SPAN
    return r, span


def sizes_call(L, name, cfg, n, n_val, rnd, span):
    fn = getattr(L.lib(), name)
    args = [ctypes.byref(cfg) if cfg is not None else None, n, n_val]
    nargs = len(L.SIGNATURES[name][1])
    if nargs >= 4:
        args.append(ctypes.byref(rnd) if rnd is not None else None)
    if nargs >= 5:
        args.append(span)
    return int(fn(*args))


def run_refusal(L, row):
    """Call row["entry"] as the row says; -> its return code."""
    t = TRAINERS[row["trainer"]]
    name = row["entry"]
    cfg = None if row["cfg"] is None else make_config(L, row["trainer"], row["cfg"])
    n, n_val = row["n"], row["n_val"]
    rnd, span = make_random(L, cfg, n, row["options"])
    nargs = len(L.SIGNATURES[name][1])
    if name.endswith("_workspace_bytes"):
        return sizes_call(L, name, cfg, n, n_val, rnd, span)
    null = set(row["null"])
    ptr = lambda arg: None if arg in null else FAKE  # noqa: E731
    cfg_p = ctypes.byref(cfg) if cfg is not None else None
    rnd_p = ctypes.byref(rnd) if rnd is not None else None
    need = 0  # no row gets past the work-space check, the last one before the first HIP call
    if row["ws"] == "short":
        need = sizes_call(L, t["stretch"], cfg, n, n_val if name in t["train"] else 0, rnd, span) - 1
        assert need > 0, row
    if name in t["train"]:
        epochs = ctypes.c_int32(0)
        args = [cfg_p, n, ptr("d_x"), ptr("d_y"), n_val, ptr("d_x_val"), ptr("d_y_val"), ptr("d_rates"), 3, 0,
                row["patience"], ptr("d_params")]
        if t["stats"]:
            args.append(ptr("d_stats"))
        args += [ptr("d_train_loss"), ptr("d_val_loss"), ctypes.byref(epochs), ptr("d_ws"), need, FAKE]
        base = len(args)
    else:
        args = [cfg_p, n, ptr("d_x"), ptr("d_y"), ptr("d_params"), ptr("d_loss"), ptr("d_grads"), ptr("d_ws"), need,
                FAKE]
        base = len(args)
    if nargs > base:
        args.append(rnd_p)
    if nargs > base + 1:
        args.append(span)
    assert len(args) == nargs, (name, len(args), nargs)
    return int(getattr(L.lib(), name)(*args))


def takes(L, name, options):
    """Whether the entry `name` has the arguments that `options` needs."""
    nargs = len(L.SIGNATURES[name][1])
    if name.endswith("_workspace_bytes"):
        has_random, has_span = nargs >= 4, nargs >= 5
    else:
        first = L.SIGNATURES[name][1]
        has_random = first[-1] is ctypes.POINTER(L.TrainRandom) or first[-2] is ctypes.POINTER(L.TrainRandom)
        has_span = first[-2] is ctypes.POINTER(L.TrainRandom)
    if options == "none":
        return True
    if options in ("dropout", "source"):
        return has_random
    return has_span


# ---- the tables ----------------------------------------------------------------------------------------------------------

def workspace_cells(trainer):
    t = TRAINERS[trainer]
    norms = [(0, 0), (1, 1), (1, 0), (0, 1)] if t["norm"] else [(0, 0)]
    for n, n_vals in ((1, (0, 4)), (5, (0, 2, 7)), (1024, (0, 100))):
        for n_val in n_vals:
            for layers in (1, t["layers"][1]):
                for norm, pool in norms:
                    for options in ("none", "dropout", "source", "source+span"):
                        yield n, n_val, layers, norm, pool, options


def cell_changes(trainer, layers, norm, pool):
    t = TRAINERS[trainer]
    ch = {t["layers"][0]: layers}
    if t["norm"]:
        ch[t["norm"]] = norm
        ch[t["norm"].rsplit(".", 1)[0] + ".pool" if "." in t["norm"] else "pool"] = pool
    return ch


def workspace_row(L, trainer, cell):
    t = TRAINERS[trainer]
    n, n_val, layers, norm, pool, options = cell
    cfg = make_config(L, trainer, cell_changes(trainer, layers, norm, pool))
    rnd, span = make_random(L, cfg, n, options)
    older = sizes_call(L, t["older"], cfg, n, n_val, None, 0) if t["older"] else None
    older_random = sizes_call(L, t["older_random"], cfg, n, n_val, rnd, 0) if t["older_random"] and span == 0 else None
    grads = sizes_call(L, t["grads_bytes"], cfg, n, n_val, rnd, 0) if t["grads_bytes"] and span == 0 else None
    return [n, n_val, layers, norm, pool, options, sizes_call(L, t["stretch"], cfg, n, n_val, rnd, span), older,
            older_random, grads]


def refusal_cases(L, trainer):
    """Every refusal of the trainer's public entries that happens before the first HIP call, without its rc."""
    t = TRAINERS[trainer]
    sizes = [e for e in (t["older"], t["older_random"], t["stretch"], t["grads_bytes"]) if e]
    bn = {t["norm"]: 1} if t["stats"] else {}

    def row(entry, case, fields=(), cfg={}, n=N, n_val=N_VAL, options="none", patience=-1, null=(), ws="none"):
        if entry in t["grads"]:
            n_val = 0
        return dict(trainer=trainer, entry=entry, case=case, fields=list(fields), cfg=cfg, n=n, n_val=n_val,
                    options=options, patience=patience, null=list(null), ws=ws)

    for entry in sizes + t["train"] + t["grads"]:
        is_train, is_grads = entry in t["train"], entry in t["grads"]
        yield row(entry, "null_config", cfg=None)
        for fields, changes, options in LIMITS[trainer]:
            if takes(L, entry, options):
                yield row(entry, "limit", fields, {k: v for k, v in changes.items() if not k.startswith("_")},
                          n=changes.get("_n", N), options=options)
        if not is_grads:
            yield row(entry, "n_val_past_limit", n_val=1025)
            if takes(L, entry, "source+span"):
                yield row(entry, "span_one", options="span_one")
                yield row(entry, "span_without_source", options="span_alone")
        if is_train or is_grads:
            yield row(entry, "null_params", null=["d_params"])
            yield row(entry, "ws_short", ws="short")
        if is_train:
            yield row(entry, "null_validation", null=["d_x_val"])
            yield row(entry, "null_validation", null=["d_y_val"])
            yield row(entry, "null_validation", null=["d_val_loss"])
            yield row(entry, "patience_without_validation", n_val=0, patience=2)
            if t["stats"]:
                yield row(entry, "null_stats", cfg=dict(bn), null=["d_stats"])


def build(L):
    out = {"workspace": {}, "refusals": []}
    for trainer in TRAINERS:
        out["workspace"][trainer] = [workspace_row(L, trainer, c) for c in workspace_cells(trainer)]
        for r in refusal_cases(L, trainer):
            r["rc"] = run_refusal(L, r)
            out["refusals"].append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=str(HERE.parents[1]),
                    help="built checkout whose onset_fingerprinting_amd is read (default: this one)")
    a = ap.parse_args()
    out = build(load_lib(a.package_root))
    bad = [r for rows in out["workspace"].values() for r in rows if r[6] <= 0]
    assert not bad, f"work-space table holds refused rows: {bad[:3]}"
    ok = [r for r in out["refusals"] if r["rc"] == 0 or r["rc"] > 0 and r["entry"].endswith("_workspace_bytes")]
    assert not ok, f"refusal rows that were not refused: {ok[:3]}"
    lines = ["{", ' "workspace": {']
    lines.append(",\n".join(f'  "{t}": [\n' + ",\n".join("   " + json.dumps(r) for r in rows) + "\n  ]"
                            for t, rows in out["workspace"].items()))
    lines += [" },", ' "refusals": [', ",\n".join("  " + json.dumps(r) for r in out["refusals"]), " ]", "}"]
    OUT.write_text("\n".join(lines) + "\n")
    print(f"wrote {OUT}: {sum(len(v) for v in out['workspace'].values())} sizes, {len(out['refusals'])} refusals")


if __name__ == "__main__":
    main()
