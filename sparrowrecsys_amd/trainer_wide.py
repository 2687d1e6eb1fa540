"""``trainer_wide.fit(model, ...)`` for ``WideNDeep`` -- ``EmbeddingMLP``'s deep stack plus a wide term in the head whose parameter row is
chosen by a hash of two id columns (``crossed_column([movieId, userRatedMovie1], cross_buckets)``, WideNDeep.py:72-73) -- trained with Adam
under the rules of :mod:`trainer` (DESIGN.md sections 5.12 and 5.20).

:func:`train_host` is the DEFINITION, in numpy with a fixed operation order; ``sprk_train_wide_fit`` (csrc/k_train_wide.h,
csrc/api_train_wide.h) computes the same bits on the device.  The arithmetic is the trainer's own, through the trainer's own functions:
float32, every product and sum rounded on its own, no fused multiply-add, sums from ``+0`` in index order, ``sigmoid_def``, the two-level
gradient sums (a tile's samples, then the tiles), Adam over every element on every step -- the ``cross_buckets`` wide rows included, as
Keras' Adam moves them --, ``alpha_t`` in doubles on the host, ``order`` applied once; non-finite inputs and ids outside the vocabulary
are errors found before the first step.  What this graph adds (``H = hidden[-1]``; ``ids [N, 11]`` in ``model.id_columns`` order: the ten
``EMB_KEYS`` columns, then ``userRatedMovie1``, which has a vocabulary -- ``rated_buckets`` -- and no table; ``dense [N, 7]``):

* ``bucket = cross_bucket_host(movieId, userRatedMovie1, cross_buckets)``: the FingerprintCat64 chain from the key ``0xDECAFCAFFE``;
* the deep stack as ``trainer.forward_host`` up to the last hidden activation ``a``; ``S = ((+0 + a_0 k_0) + a_1 k_1) + ...`` over
  ``head/kernel[:H]`` in row order;
* ``cross_dim == 0`` (the reference's ``indicator_column``): ``logit = (S + head/kernel[H + bucket]) + head/bias`` -- the indicator's product
  with 1 is exact and its zero rows are skipped; the rows ``head/kernel[H:]`` are trained like a table of width 1 keyed by ``bucket``;
* ``cross_dim > 0`` (an ``embedding_column``; BASELINE config 5): the same chain goes on over ``e = emb/cross[bucket]`` and
  ``head/kernel[H : H + cross_dim]``, then the bias; ``emb/cross`` row ``bucket`` receives ``dl head/kernel[H + d]``, the product rounded once;
* ``dl = (p - y) / n``; a cross row's gradient is summed over the samples that hashed to it, within a tile from ``+0``, then the tiles from
  ``+0``; a row no sample hashed to gets ``+0`` (and still moves with its moments).
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np

from . import trainer as _T
from .trainer import (DEFAULT_BATCH, LDS_BYTES, TrainResult, _back, _check_args, _check_order, _dense, _error_message, _grad_bias, _grad_kernel, _grad_table,
                      adam_alpha, adam_constants, adam_step, sigmoid_def)

MAX_COLS, MAX_LAYERS, MAX_X, MAX_WIDTH = _T.MAX_COLS, _T.MAX_LAYERS, _T.MAX_X, _T.MAX_WIDTH
MAX_CROSS_DIM = 64                                                    # SPRK_TRAIN_WIDE_MAX_CROSS_DIM (BASELINE config 5 has 32)
TILE_WIDE = 4                                                         # default_tile(): from the tile sweep in docs/train_wide_results.md
MAX_ROWS = (1 << 31) - 1                                              # the schedule's key holds a row in 32 bits
CROSS_KEY = 0xDECAFCAFFE
_F = np.float32

WideFamily = namedtuple("WideFamily", "columns tables emb_dim xcol xsub n_dense widths layers cross_a cross_b cross_buckets cross_dim")
WideFamily.__doc__ = """``trainer.Family``'s fields for the deep half -- ``columns`` holds all eleven id columns, ``tables`` the ten trained ones, in
column order --, then the cross: the id columns it hashes (``cross_a`` = ``movieId``, ``cross_b`` = ``userRatedMovie1``, the last column,
which has no table), ``cross_buckets`` and ``cross_dim`` (0 = the indicator form)."""


def family_of(model) -> WideFamily:
    """The trainer's view of a ``WideNDeep`` (that class itself: a subclass may compute another graph)."""
    from . import models as M
    if type(model) is not M.WideNDeep:
        raise NotImplementedError("trainer_wide trains WideNDeep, not %s" % type(model).__name__)
    D = int(model.emb_dim)
    rows, n_x = model._deep_blocks_order(), model._deep_in()
    xcol, xsub = [None] * n_x, [None] * n_x
    for c, k in enumerate(model.EMB_KEYS):
        for d in range(D):
            xcol[rows[k + "_embedding"] + d], xsub[rows[k + "_embedding"] + d] = c, d
    for j, k in enumerate(model.numeric_keys):
        xcol[rows[k]], xsub[rows[k]] = -1, j
    cols = [(c.key, c.kind, int(c.vocab)) for c in model.id_columns]
    keys = [c[0] for c in cols]
    fam = WideFamily(cols, ["emb/" + k for k in model.EMB_KEYS], D, xcol, xsub, len(model.numeric_keys), [int(h) for h in model.hidden],
                     ["dense%d" % i for i in range(len(model.hidden))] + ["head"], keys.index("movieId"), keys.index("userRatedMovie1"),
                     int(model.cross_buckets), int(model.cross_dim))
    _check_family(fam)
    return fam


def _check_family(fam: WideFamily):
    C = len(fam.columns)
    if not (2 <= C <= MAX_COLS and len(fam.tables) == C - 1):
        raise ValueError("trainer_wide takes up to %d id columns with a table and one more without" % (MAX_COLS - 1))
    _T._check_family(fam)
    if fam.cross_b != C - 1 or not 0 <= fam.cross_a < fam.cross_b or any(c == fam.cross_b for c in fam.xcol):
        raise ValueError("the cross hashes a column that has a table with the last column, which has a vocabulary, no table and no input row")
    if not 0 <= fam.cross_dim <= MAX_CROSS_DIM:
        raise ValueError("cross_dim = %d: the cross is an indicator (0) or an embedding of up to %d" % (fam.cross_dim, MAX_CROSS_DIM))
    if fam.cross_buckets < 1:
        raise ValueError("cross_buckets = %d must be >= 1" % fam.cross_buckets)
    deep_rows = sum(v for _, _, v in fam.columns[:-1])
    if deep_rows + fam.cross_buckets >= MAX_ROWS:
        raise ValueError("the deep tables' %d rows + cross_buckets = %d: the schedule's key holds fewer than 2^31 - 1 rows" % (deep_rows, fam.cross_buckets))


def param_names(fam: WideFamily):
    """Every trained array -- all of ``WideNDeep.weight_shapes()`` -- in the order of the device's flat parameter vector: the ten tables, the
    hidden layers' kernels and biases, ``head/bias`` BEFORE ``head/kernel`` (so the Dense parameters, ``head/kernel[:H + cross_dim]``
    included, are one contiguous stretch and the indicator form's ``cross_buckets`` wide rows, which are trained like a table, follow it
    while ``head/kernel`` stays one array), then ``emb/cross`` in the embedding form."""
    out = list(fam.tables)
    for name in fam.layers[:-1]:
        out += [name + "/kernel", name + "/bias"]
    return out + ["head/bias", "head/kernel"] + (["emb/cross"] if fam.cross_dim else [])


def param_shapes(fam: WideFamily):
    s = _T.param_shapes(fam)                                           # (zip stops at the ten tables)
    s["head/kernel"] = (fam.widths[-1] + (fam.cross_dim or fam.cross_buckets), 1)
    if fam.cross_dim:
        s["emb/cross"] = (fam.cross_buckets, fam.cross_dim)
    return s


def default_tile(fam: WideFamily) -> int:
    """The ``tile`` of a fit that names none: 4 where a layer (the input included) is wider than 32 -- the tile sweep of
    docs/train_wide_results.md at the reference's 107-128-128 stack, in both cross forms: 515 us a step at tile 4, 562 at 8, 627 at 2 --,
    else ``trainer.default_tile``'s 16 for a narrow stack, which was not measured for this graph."""
    return _T.TILE_NARROW if max([len(fam.xcol)] + list(fam.widths)) <= _T.NARROW else TILE_WIDE


def lds_bytes(fam: WideFamily, tile: int) -> int:
    """The LDS of one workgroup of the step kernel: ``trainer.lds_bytes`` and the tile's ``emb/cross`` rows."""
    return _T.lds_bytes(fam, tile) + 4 * int(tile) * fam.cross_dim


# ---------------------------------------------------------------- the definition

def cross_bucket_host(a, b, buckets: int):
    """``FingerprintCat64(FingerprintCat64(0xDECAFCAFFE, a), b) % buckets`` per element, ``a`` and ``b`` sign-extended to 64 bits: the chain of
    ``k_tile_forward.h`` ``cross_bucket`` and ``oracle.farmhash64.cross_hashed``, in numpy uint64 (products wrap).  -> int64."""
    mul, s47 = np.uint64(0xc6a4a7935bd1e995), np.uint64(47)
    mix = lambda x: x ^ (x >> s47)

    def cat(fp1, fp2):
        r = fp1 ^ mul
        r = r ^ (mix(fp2 * mul) * mul)
        r = r * mul
        return mix(mix(r) * mul)
    with np.errstate(over="ignore"):
        h = np.full(np.shape(a), CROSS_KEY, dtype=np.uint64)
        for x in (a, b):
            h = cat(h, np.asarray(x).astype(np.int64).astype(np.uint64))
        return (h % np.uint64(buckets)).astype(np.int64)


def buckets_of(fam: WideFamily, ids):
    return cross_bucket_host(ids[:, fam.cross_a], ids[:, fam.cross_b], fam.cross_buckets)


def forward_host(fam: WideFamily, w, ids, dense, keep=None):
    """The definition's probabilities ``[n]`` for packed rows; ``keep`` (a list) receives the input, every activation, then the buckets and
    (embedding form) the gathered ``emb/cross`` rows."""
    a = _T.input_rows(fam, w, ids, dense)
    acts = [a]
    H = fam.widths[-1]
    hk, hb = w["head/kernel"], w["head/bias"]
    bucket = buckets_of(fam, ids)
    with np.errstate(all="ignore"):
        for name in fam.layers[:-1]:
            z = _dense(a, w[name + "/kernel"], w[name + "/bias"])
            a = np.where(z > 0, z, _F(0.0)).astype(_F)
            acts.append(a)
        if fam.cross_dim:
            e = w["emb/cross"][bucket]
            logit = _dense(np.concatenate([a, e], axis=1), hk[:H + fam.cross_dim], hb)[:, 0]
        else:
            e = None
            S = _dense(a, hk[:H], np.zeros(1, dtype=_F))[:, 0]         # (the chain starts at +0 and is never -0: adding +0 changes no bit)
            logit = (S + hk[H + bucket, 0]) + hb[0]
    if keep is not None:
        keep.extend(acts + [bucket, e])
    return sigmoid_def(logit)


def step_gradients(fam: WideFamily, w, ids, dense, labels, tile: Optional[int] = None):
    """One step's gradients: ``({name: gradient}, p)`` for the batch ``(ids, dense, labels)`` under the weights ``w``."""
    ids, dense, labels = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F), np.asarray(labels, dtype=_F)
    n, tile = ids.shape[0], default_tile(fam) if tile is None else int(tile)
    kept = []
    p = forward_host(fam, w, ids, dense, kept)
    acts, bucket, e = kept[:-2], kept[-2], kept[-1]
    H, hk = fam.widths[-1], w["head/kernel"]
    g = {}
    with np.errstate(all="ignore"):
        dl = ((p - labels) / _F(n)).astype(_F)[:, None]
        a = acts[-1]
        g["head/bias"] = _grad_bias(dl, tile)
        if fam.cross_dim:
            g["head/kernel"] = np.concatenate([_grad_kernel(a, dl, tile), _grad_kernel(e, dl, tile)])
            g["emb/cross"] = _grad_table(bucket, (dl * hk[H:, 0][None, :]).astype(_F), fam.cross_buckets, tile)
        else:
            g["head/kernel"] = np.concatenate([_grad_kernel(a, dl, tile), _grad_table(bucket, dl, fam.cross_buckets, tile)])
        da = _back(hk[:H], dl)
        dz = np.where(a > 0, da, _F(0.0)).astype(_F)
        for li in range(len(fam.layers) - 2, -1, -1):                  # trainer.step_gradients' loop, below the head
            name, a = fam.layers[li], acts[li]
            g[name + "/kernel"] = _grad_kernel(a, dz, tile)
            g[name + "/bias"] = _grad_bias(dz, tile)
            da = _back(w[name + "/kernel"], dz)
            dz = np.where(a > 0, da, _F(0.0)).astype(_F) if li else da
        for c, (tab, col) in enumerate(zip(fam.tables, fam.columns)):
            ks = [k for k in range(len(fam.xcol)) if fam.xcol[k] == c]
            ks.sort(key=lambda k: fam.xsub[k])
            g[tab] = _grad_table(ids[:, c], dz[:, ks], col[2], tile)
    return g, p


def validate_host(fam: WideFamily, ids, dense, labels):
    """The trainer's checks before the first step, over all eleven id columns: ``userRatedMovie1`` outside ``[0, rated_buckets)`` is error
    kind 1, so a bucket is only ever hashed from valid ids."""
    _T.validate_host(fam, ids, dense, labels)


def _copy_state(fam, weights, state):
    names, shapes = param_names(fam), param_shapes(fam)
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else a
    w = {}
    for k in names:
        a = np.array(host(weights[k]), dtype=_F)
        if a.shape != shapes[k]:
            raise ValueError("weight %r has shape %s, expected %s" % (k, a.shape, shapes[k]))
        w[k] = a
    if state is None:
        return w, {k: np.zeros_like(w[k]) for k in names}, {k: np.zeros_like(w[k]) for k in names}, 0
    m, v, step = state
    return w, {k: np.array(host(m[k]), dtype=_F) for k in names}, {k: np.array(host(v[k]), dtype=_F) for k in names}, int(step)


def train_host(fam: WideFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
               order=None, tile: Optional[int] = None, state=None) -> TrainResult:
    """The definition on packed host arrays, with ``trainer.train_host``'s arguments and returns: ``ids [N, 11]`` int32 in
    ``model.id_columns`` order, ``dense [N, F]`` float32, ``labels [N]`` float32; ``order`` a permutation of the rows, applied once;
    ``state = (m, v, step)`` continues an earlier fit.  Nothing is changed when a check fails."""
    from .metrics import evaluate_scores
    tile = default_tile(fam) if tile is None else int(tile)
    _check_args(batch_size, epochs, learning_rate, tile)
    ids, dense, labels = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F), np.asarray(labels, dtype=_F).reshape(-1)
    N, B = ids.shape[0], int(batch_size)
    dense = dense.reshape(N, fam.n_dense)
    if ids.shape != (N, len(fam.columns)) or labels.shape != (N,):
        raise ValueError("ids must be [N, %d], dense [N, %d] and labels [N]" % (len(fam.columns), fam.n_dense))
    w, m, v, step = _copy_state(fam, weights, state)
    validate_host(fam, ids, dense, labels)
    if order is not None:
        order = _check_order(order, N)
        ids, dense, labels = ids[order], dense[order], labels[order]
    history, p = [], np.zeros(N, dtype=_F)
    for _ in range(int(epochs)) if N else []:
        for b0 in range(0, N, B):
            b1 = min(N, b0 + B)
            g, p[b0:b1] = step_gradients(fam, w, ids[b0:b1], dense[b0:b1], labels[b0:b1], tile)
            step += 1
            alpha = adam_alpha(learning_rate, step)
            for k in w:
                adam_step(w[k], m[k], v[k], g[k], alpha)
        history.append(evaluate_scores(labels.astype(np.float64), p))
    return TrainResult(w, m, v, step, history, p)


# ---------------------------------------------------------------- the device

def _flatten(fam, arrays, dev):
    import torch
    parts = []
    for k in param_names(fam):
        a = arrays[k]
        a = a.detach().to(dev, torch.float32) if hasattr(a, "detach") else torch.from_numpy(np.ascontiguousarray(a, dtype=_F)).to(dev)
        parts.append(a.reshape(-1))
    return torch.cat(parts).contiguous()


def _unflatten(fam, flat):
    out, at, shapes = {}, 0, param_shapes(fam)
    for k in param_names(fam):
        n = int(np.prod(shapes[k]))
        out[k] = flat[at:at + n].reshape(shapes[k])
        at += n
    return out


def _model_struct(fam):
    from . import _lib as L
    s = L.TrainWideModel()
    s.n_cols, s.n_dense, s.emb_dim, s.n_x, s.n_layers = len(fam.columns), fam.n_dense, fam.emb_dim, len(fam.xcol), len(fam.widths)
    for c, (_, kind, vocab) in enumerate(fam.columns):
        s.vocab[c], s.genre[c] = vocab, 1 if kind == "genre" else 0
    for i, h in enumerate(fam.widths):
        s.width[i] = h
    for k, (c, x) in enumerate(zip(fam.xcol, fam.xsub)):
        s.xcol[k], s.xsub[k] = c, x
    s.cross_a, s.cross_b, s.cross_buckets, s.cross_dim = fam.cross_a, fam.cross_b, fam.cross_buckets, fam.cross_dim
    return s


def train_device(fam: WideFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
                 order=None, tile: Optional[int] = None, state=None, device=None, workspace=None, num_thresholds: int = 200) -> TrainResult:
    """:func:`train_host` on the device (``sprk_train_wide_fit``): the same bits in every weight, ``m``, ``v`` and ``p``; the history through
    ``metrics.DeviceMetrics`` (accuracy and both AUCs bit for bit, the loss within a float64 sum's rounding).  Arguments and returns are
    ``trainer.train_device``'s; the whole fit is enqueued on the current stream and the one synchronisation fetches the error word."""
    import ctypes as C

    import torch

    from . import _lib as L
    from .metrics import DeviceMetrics
    tile = default_tile(fam) if tile is None else int(tile)
    _check_args(batch_size, epochs, learning_rate, tile)
    if not torch.cuda.is_available():
        raise RuntimeError("train_device needs a HIP device: no HIP device is visible (train_host is the host definition)")
    lib = L.load_library()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n_c = len(fam.columns)

    def up(a, dt):
        if hasattr(a, "detach"):
            return a.detach().to(dev).to(dt).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.float32: _F}[dt])).to(dev)
    with torch.cuda.device(dev):
        ids, labels = up(ids, torch.int32), up(labels, torch.float32).reshape(-1)
        N, B, E = int(ids.shape[0]), int(batch_size), int(epochs)
        dense = up(dense, torch.float32).reshape(N, fam.n_dense)
        if tuple(ids.shape) != (N, n_c) or int(labels.numel()) != N:
            raise ValueError("ids must be [N, %d], dense [N, %d] and labels [N]" % (n_c, fam.n_dense))
        if N * n_c >= (1 << 31) - 1:
            raise ValueError("N x id columns = %d: the schedule's offsets hold fewer than 2^31 - 1 entries" % (N * n_c))
        if lds_bytes(fam, tile) > LDS_BYTES:
            raise ValueError("tile = %d needs %d bytes of LDS for this model, more than %d" % (tile, lds_bytes(fam, tile), LDS_BYTES))
        if order is not None:
            if hasattr(order, "detach"):
                o64 = order.detach().to(dev).to(torch.int64).reshape(-1)
                if int(o64.numel()) != N or not bool((torch.sort(o64).values == torch.arange(N, device=dev)).all()):
                    raise ValueError("order must be a permutation of 0 .. N - 1")
            else:
                o64 = torch.from_numpy(_check_order(order, N)).to(dev)
            order_t = o64.to(torch.int32).contiguous()
        shapes = param_shapes(fam)
        for k in param_names(fam):
            if tuple(weights[k].shape) != shapes[k]:
                raise ValueError("weight %r has shape %s, expected %s" % (k, tuple(weights[k].shape), shapes[k]))
        params = _flatten(fam, weights, dev)                                           # (a copy: the caller's arrays stay as they are)
        if state is None:
            m, v, step = torch.zeros_like(params), torch.zeros_like(params), 0
        else:
            m, v, step = _flatten(fam, state[0], dev), _flatten(fam, state[1], dev), int(state[2])
        steps = (N + B - 1) // B if N else 0
        alphas = np.array([adam_alpha(learning_rate, step + 1 + i) for i in range(E * steps)] + [0.0], dtype=_F)
        t_alpha = torch.from_numpy(alphas).to(dev)
        p = torch.zeros(max(E, 1) * max(N, 1), dtype=torch.float32, device=dev)
        word = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ms = _model_struct(fam)
        need = int(lib.sprk_train_wide_workspace_bytes(C.byref(ms), N, B, tile))
        if workspace is None:
            workspace = torch.empty(max(need, 16) // 8 + 2, dtype=torch.int64, device=dev)
        c1, c2, eps = adam_constants()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if E and N:
            L.check(lib.sprk_train_wide_fit(C.byref(ms), ptr(ids), ptr(dense) if fam.n_dense else None, ptr(labels), ptr(order_t) if order is not None else None,
                                            N, B, tile, E, ptr(t_alpha), float(c1), float(c2), float(eps), ptr(params), ptr(m), ptr(v), ptr(p), ptr(word),
                                            ptr(workspace), workspace.numel() * workspace.element_size(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        seen = labels if order is None else labels[o64]
        dms = []
        for e in range(E if N else 0):
            dm = DeviceMetrics(num_thresholds, device=dev)
            dm.update(p[e * N:(e + 1) * N], seen)
            dms.append(dm)
        err = int(word.cpu()[0])                                                       # the one synchronisation
        if err != -1:
            raise ValueError(_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
        history = [dm.result() for dm in dms]
    last = p[(E - 1) * N:E * N] if E and N else p[:0]
    return TrainResult(_unflatten(fam, params), _unflatten(fam, m), _unflatten(fam, v), step + E * steps, history, last if E else torch.zeros(N, dtype=torch.float32, device=dev))


def fit(model, x, y=None, batch_size: int = 4096, epochs: int = 5, learning_rate: float = 0.001, order=None, tile: Optional[int] = None):
    """``CTRModel.fit`` for a ``WideNDeep``: the same arguments (a dict of columns with ``"label"`` or ``y``, or an iterable of ``(features,
    labels)`` batches) and the same return value (per epoch ``[loss, accuracy, roc_auc, pr_auc]``); the trained weights are set on
    ``model`` and Adam's moments kept in ``model._fit_state``, so a second call continues.  This function is the entry:
    ``WideNDeep.fit`` itself still raises ``NotImplementedError``, and ``trainer.family_of`` and ``CTRModel.fit`` are as they were
    (DESIGN.md section 5.20 says what the one-line dispatch waits on)."""
    import sys
    fam = family_of(model)
    return model._fit_with(sys.modules[__name__], fam, x, y, batch_size, epochs, learning_rate, order, tile)
