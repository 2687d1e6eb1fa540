"""``trainer_tower.fit(model, ...)`` for ``NeuralCF(arch=2)`` -- the reference's ``neural_cf_model_2`` (NeuralCF.py:57-70): a Dense/ReLU tower over the
movie embedding, one over the user embedding, their ``Dot``, ``Dense(1, sigmoid)`` -- trained with Adam under the rules of :mod:`trainer`
(DESIGN.md sections 5.12 and 5.23); and :func:`towers`, which turns the trained towers into the item and user vectors of an ``als.ALSModel``:
samples -> trained towers -> top-K lists -> ranking metrics without leaving HBM.

:func:`train_host` is the DEFINITION, in numpy with a fixed operation order; ``sprk_train_tower_fit`` (csrc/k_train_tower.h,
csrc/api_train_tower.h) computes the same bits on the device.  The arithmetic is the trainer's own, through the trainer's own functions: float32,
every product and sum rounded on its own, no fused multiply-add, sums from ``+0`` in index order, ReLU ``z if z > 0 else +0``, ``sigmoid_def``, the
two-level gradient sums (a tile's samples, then the tiles), Adam over every element of every array on every step, ``alpha_t`` in doubles on the
host, ``order`` applied once; ids outside the vocabulary and non-finite labels are errors found before the first step.  What this graph adds
(``D = emb_dim``, ``H = hidden[-1]``; ``ids [N, 2]`` = movieId, userId; there are no numerics, ``dense`` is ``[N, 0]``):

* each tower is ``a <- relu(_dense(a, W, b))`` per layer from its table's row: ``item{i}`` over ``emb/movieId``, ``user{i}`` over ``emb/userId``,
  the same widths in both;
* ``dot`` is ``als.predict_host``'s: ``acc = acc + it[d] * us[d]`` from ``0.0f`` in index order -- so a pair's dot in training, ``sprk_als_predict``
  on the exported vectors and the score ``sprk_als_topk`` sorts by are the same bits;
* ``logit = _dense(dot[:, None], head/kernel, head/bias)[:, 0]``, ``p = sigmoid_def(logit)``;
* backwards ``dlogit = (p - y) / n``; the head's gradients as a Dense unit's over ``dot``; ``ddot = _back(head/kernel, dlogit)``; the item tower's
  last activation receives ``ddot * user_out``, the user tower's ``ddot * item_out``, each under its own ReLU mask (``a > 0``); each tower then
  walks down its layers as ``trainer.step_gradients`` does; the two tables through ``_grad_table`` over their column;
* a NaN that reaches a stored value (``p``, a weight, ``m``, ``v``) is stored as the quiet NaN ``0x7fc00000``, as in :mod:`trainer_fm`: a dot can
  overflow to ``inf``, and ``0 * inf`` follows.

:func:`tower_rows_host` / :func:`tower_rows_device` (``sprk_tower_rows``) send every row of one table through its tower by the forward's own
statements; :func:`towers` wraps both sides' rows as a :class:`TowerModel`, whose ``predict`` / ``recommend_for_users`` / ``recommend_for_items``
/ ``evaluate_ranking`` are ``als.ALSModel``'s.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np

from . import als as _A
from . import trainer as _T
from .trainer import (DEFAULT_BATCH, LDS_BYTES, TrainResult, _back, _check_args, _check_order, _dense, _error_message, _grad_bias, _grad_kernel, _grad_table,
                      adam_alpha, adam_constants, adam_step, sigmoid_def)
from .trainer_fm import QNAN, _canonical

MAX_LAYERS, MAX_WIDTH, MAX_DIM = _T.MAX_LAYERS, _T.MAX_WIDTH, _T.MAX_X // 2
DEFAULT_TILE = 16                                                     # chosen from the tile sweep in docs/train_tower_results.md
ROWS_TILE = 64                                                        # tower_rows_device: table rows per workgroup pass
MAX_ROWS = (1 << 31) - 1                                              # the schedule's key holds a row in 32 bits
SIDES = {"item": 0, "user": 1}
_F = np.float32


class TowerFamily(namedtuple("TowerFamily", "columns emb_dim hidden")):
    """``columns``: ``("movieId", "id", vocab)`` and ``("userId", "id", vocab)``, the id columns of ``pack_device``; ``emb_dim``; ``hidden``: the
    widths both towers share (``models.NeuralCF.weight_shapes()``)."""
    __slots__ = ()


def make_family(movie_vocab: int, user_vocab: int, emb_dim: int, hidden) -> TowerFamily:
    fam = TowerFamily([("movieId", "id", int(movie_vocab)), ("userId", "id", int(user_vocab))], int(emb_dim), [int(h) for h in hidden])
    _check_family(fam)
    return fam


def family_of(model) -> TowerFamily:
    """The trainer's view of a ``NeuralCF(arch=2)`` (that class itself: a subclass may compute another graph)."""
    from . import models as M
    if type(model) is not M.NeuralCF or model.arch != 2:
        raise NotImplementedError("trainer_tower trains NeuralCF(arch=2), not %s%s" % (type(model).__name__, "(arch=%r)" % model.arch if hasattr(model, "arch") else ""))
    return make_family(model.movie_buckets, model.user_buckets, model.emb_dim, model.hidden)


def family_from_weights(w) -> TowerFamily:
    """The family a weight dict of :func:`param_names` has the shapes of."""
    L = 0
    while "item%d/kernel" % L in w:
        L += 1
    return make_family(w["emb/movieId"].shape[0], w["emb/userId"].shape[0], w["emb/movieId"].shape[1], [w["item%d/kernel" % i].shape[1] for i in range(L)])


def _check_family(fam: TowerFamily):
    ok = (1 <= len(fam.hidden) <= MAX_LAYERS and all(1 <= h <= MAX_WIDTH for h in fam.hidden) and 1 <= fam.emb_dim and 2 * fam.emb_dim <= _T.MAX_X and
          len(fam.columns) == 2 and all(v >= 1 for _, _, v in fam.columns))
    if not ok:
        raise ValueError("trainer_tower takes 1 to %d hidden layers of up to %d units per tower, 2 x emb_dim up to %d and two vocabularies of at least 1 row" %
                         (MAX_LAYERS, MAX_WIDTH, _T.MAX_X))
    if [(k, kind) for k, kind, _ in fam.columns] != [("movieId", "id"), ("userId", "id")]:
        raise ValueError("the id columns are movieId and userId, in this order")
    if sum(v for _, _, v in fam.columns) >= MAX_ROWS:
        raise ValueError("the tables' %d rows: the schedule's key holds fewer than 2^31 - 1 rows" % sum(v for _, _, v in fam.columns))


def param_names(fam: TowerFamily):
    """Every trained array -- all of ``NeuralCF(arch=2).weight_shapes()`` -- in the order of the device's flat parameter vector."""
    out = ["emb/movieId", "emb/userId"]
    for side in ("item", "user"):
        for i in range(len(fam.hidden)):
            out += ["%s%d/kernel" % (side, i), "%s%d/bias" % (side, i)]
    return out + ["head/kernel", "head/bias"]


def param_shapes(fam: TowerFamily):
    s = {"emb/" + k: (v, fam.emb_dim) for k, _, v in fam.columns}
    for side in ("item", "user"):
        fan = fam.emb_dim
        for i, h in enumerate(fam.hidden):
            s["%s%d/kernel" % (side, i)], s["%s%d/bias" % (side, i)] = (fan, h), (h,)
            fan = h
    s["head/kernel"], s["head/bias"] = (1, 1), (1,)
    return s


def default_tile(fam: TowerFamily) -> int:
    """The ``tile`` of a fit that names none: ``DEFAULT_TILE``, halved until the tile fits the LDS (docs/train_tower_results.md has the sweep)."""
    tile = DEFAULT_TILE
    while tile > 1 and lds_bytes(fam, tile) > LDS_BYTES:
        tile //= 2
    return tile


def _round4(floats: int) -> int:
    return (int(floats) + 3) & ~3


def lds_bytes(fam: TowerFamily, tile: int) -> int:
    """The LDS of one workgroup of the step kernel, every part rounded up to 16 bytes: the tile's gathered rows ``[tile][2 D]``, every activation of
    both towers, ``dot`` and ``dlogit``, and two gradient buffers that hold both towers' widest layer side by side."""
    t = int(tile)
    floats = _round4(t * 2 * fam.emb_dim) + 2 * sum(_round4(t * h) for h in fam.hidden) + 2 * _round4(t) + 2 * _round4(t * 2 * max(fam.hidden))
    return 4 * floats


def rows_lds_bytes(fam: TowerFamily, tile: int) -> int:
    """The LDS of one workgroup of ``sprk_tower_rows``: two buffers ``[tile][the widest of emb_dim and the layers]``."""
    return 4 * 2 * _round4(int(tile) * max([fam.emb_dim] + list(fam.hidden)))


# ---------------------------------------------------------------- the definition

def _relu(z):
    return np.where(z > 0, z, _F(0.0)).astype(_F)


def _tower(fam: TowerFamily, w, side: str, a, acts=None):
    """``a`` through the side's layers; ``acts`` (a list) receives the input and every activation."""
    if acts is not None:
        acts.append(a)
    for i in range(len(fam.hidden)):
        a = _relu(_dense(a, w["%s%d/kernel" % (side, i)], w["%s%d/bias" % (side, i)]))
        if acts is not None:
            acts.append(a)
    return a


def _sdot(it, us):
    """``als.predict_host``'s dot: from ``0.0f`` in index order, every product and sum rounded on its own."""
    acc = np.zeros(it.shape[0], dtype=_F)
    for d in range(it.shape[1]):
        acc = acc + it[:, d] * us[:, d]
    return acc


def forward_host(fam: TowerFamily, w, ids, dense=None, keep: Optional[dict] = None):
    """The definition's probabilities ``[n]`` for packed rows; ``keep`` (a dict) receives every intermediate the backward pass reads."""
    ids = np.asarray(ids, dtype=np.int32).reshape(-1, 2)
    item_acts, user_acts = [], []
    with np.errstate(all="ignore"):
        it = _tower(fam, w, "item", np.asarray(w["emb/movieId"], dtype=_F)[ids[:, 0]], item_acts)
        us = _tower(fam, w, "user", np.asarray(w["emb/userId"], dtype=_F)[ids[:, 1]], user_acts)
        dot = _sdot(it, us)
        logit = _dense(dot[:, None], w["head/kernel"], w["head/bias"])[:, 0]
        p = sigmoid_def(logit)
    if keep is not None:
        keep.update(item=item_acts, user=user_acts, dot=dot, logit=logit)
    return _canonical(p)


def step_gradients(fam: TowerFamily, w, ids, dense, labels, tile: Optional[int] = None):
    """One step's gradients: ``({name: gradient}, p)`` for the batch ``(ids, labels)`` under the weights ``w``."""
    ids, labels = np.asarray(ids, dtype=np.int32).reshape(-1, 2), np.asarray(labels, dtype=_F)
    n, tile, L = ids.shape[0], default_tile(fam) if tile is None else int(tile), len(fam.hidden)
    k_ = {}
    p = forward_host(fam, w, ids, None, k_)
    acts = {"item": k_["item"], "user": k_["user"]}
    g = {}
    with np.errstate(all="ignore"):
        dl = ((p - labels) / _F(n)).astype(_F)[:, None]
        g["head/kernel"], g["head/bias"] = _grad_kernel(k_["dot"][:, None], dl, tile), _grad_bias(dl, tile)
        ddot = _back(w["head/kernel"], dl)
        for c, (side, other) in enumerate((("item", "user"), ("user", "item"))):
            a = acts[side][L]
            dz = np.where(a > 0, ddot * acts[other][L], _F(0.0)).astype(_F)
            for i in range(L - 1, -1, -1):
                a = acts[side][i]
                g["%s%d/kernel" % (side, i)], g["%s%d/bias" % (side, i)] = _grad_kernel(a, dz, tile), _grad_bias(dz, tile)
                da = _back(w["%s%d/kernel" % (side, i)], dz)
                dz = np.where(a > 0, da, _F(0.0)).astype(_F) if i else da
            g["emb/" + fam.columns[c][0]] = _grad_table(ids[:, c], dz, fam.columns[c][2], tile)
    return g, p


def adam_step_tower(w, m, v, g, alpha):
    """``trainer.adam_step``, then every NaN of ``w``, ``m`` and ``v`` stored as the quiet NaN."""
    adam_step(w, m, v, g, alpha)
    for a in (w, m, v):
        a[np.isnan(a)] = QNAN


def validate_host(fam: TowerFamily, ids, dense, labels):
    """The trainer's checks before the first step, with its messages."""
    _T.validate_host(fam, ids, dense, labels)


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else a


def _copy_state(fam, weights, state):
    names, shapes = param_names(fam), param_shapes(fam)
    w = {}
    for k in names:
        a = np.array(_host(weights[k]), dtype=_F)
        if a.shape != shapes[k]:
            raise ValueError("weight %r has shape %s, expected %s" % (k, a.shape, shapes[k]))
        w[k] = a
    if state is None:
        return w, {k: np.zeros_like(w[k]) for k in names}, {k: np.zeros_like(w[k]) for k in names}, 0
    m, v, step = state
    return w, {k: np.array(_host(m[k]), dtype=_F) for k in names}, {k: np.array(_host(v[k]), dtype=_F) for k in names}, int(step)


def train_host(fam: TowerFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
               order=None, tile: Optional[int] = None, state=None) -> TrainResult:
    """The definition on packed host arrays, with ``trainer.train_host``'s arguments and returns: ``ids [N, 2]`` int32 (movieId, userId), ``dense
    [N, 0]`` (or None), ``labels [N]`` float32; ``order`` a permutation of the rows, applied once; ``state = (m, v, step)`` continues an earlier
    fit.  Nothing is changed when a check fails."""
    from .metrics import evaluate_scores
    tile = default_tile(fam) if tile is None else int(tile)
    _check_args(batch_size, epochs, learning_rate, tile)
    ids, labels = np.asarray(ids, dtype=np.int32), np.asarray(labels, dtype=_F).reshape(-1)
    N, B = ids.shape[0], int(batch_size)
    dense = np.zeros((N, 0), dtype=_F) if dense is None else np.asarray(dense, dtype=_F).reshape(N, 0)
    if ids.shape != (N, 2) or labels.shape != (N,):
        raise ValueError("ids must be [N, 2], dense [N, 0] and labels [N]")
    w, m, v, step = _copy_state(fam, weights, state)
    validate_host(fam, ids, dense, labels)
    if order is not None:
        order = _check_order(order, N)
        ids, labels = ids[order], labels[order]
    history, p = [], np.zeros(N, dtype=_F)
    for _ in range(int(epochs)) if N else []:
        for b0 in range(0, N, B):
            b1 = min(N, b0 + B)
            g, p[b0:b1] = step_gradients(fam, w, ids[b0:b1], None, labels[b0:b1], tile)
            step += 1
            alpha = adam_alpha(learning_rate, step)
            for k in w:
                adam_step_tower(w[k], m[k], v[k], g[k], alpha)
        history.append(evaluate_scores(labels.astype(np.float64), p))
    return TrainResult(w, m, v, step, history, p)


def tower_rows_host(fam: TowerFamily, w, side: str) -> np.ndarray:
    """``[vocab, hidden[-1]]`` float32: every row of the side's table (``"item"``: ``emb/movieId``, ``"user"``: ``emb/userId``) through the side's
    tower, by the forward's own statements."""
    c = SIDES[side]
    with np.errstate(all="ignore"):
        return _tower(fam, w, side, np.array(_host(w["emb/" + fam.columns[c][0]]), dtype=_F))


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


def n_params(fam: TowerFamily) -> int:
    return sum(int(np.prod(s)) for s in param_shapes(fam).values())


def _model_struct(fam):
    from . import _lib as L
    s = L.TrainTowerModel()
    s.emb_dim, s.n_layers = fam.emb_dim, len(fam.hidden)
    s.vocab[0], s.vocab[1] = fam.columns[0][2], fam.columns[1][2]
    for i, h in enumerate(fam.hidden):
        s.width[i] = h
    return s


def train_device(fam: TowerFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
                 order=None, tile: Optional[int] = None, state=None, device=None, workspace=None, num_thresholds: int = 200) -> TrainResult:
    """:func:`train_host` on the device (``sprk_train_tower_fit``): the same bits in every weight, ``m``, ``v`` and ``p``; the history through
    ``metrics.DeviceMetrics`` (accuracy and both AUCs bit for bit, the loss within a float64 sum's rounding).  Arguments and returns are
    ``trainer.train_device``'s (``dense`` is ``[N, 0]`` or None); the whole fit is enqueued on the current stream and the one synchronisation
    fetches the error word.  -> ``TrainResult`` of device tensors (views of three flat vectors)."""
    import ctypes as C

    import torch

    from . import _lib as L
    from .metrics import DeviceMetrics
    tile = default_tile(fam) if tile is None else int(tile)
    _check_args(batch_size, epochs, learning_rate, tile)
    _check_family(fam)
    if not torch.cuda.is_available():
        raise RuntimeError("train_device needs a HIP device: no HIP device is visible (train_host is the host definition)")
    lib = L.load_library()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def up(a, dt):
        if hasattr(a, "detach"):
            return a.detach().to(dev).to(dt).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.float32: _F}[dt])).to(dev)
    with torch.cuda.device(dev):
        ids, labels = up(ids, torch.int32), up(labels, torch.float32).reshape(-1)
        N, B, E = int(ids.shape[0]), int(batch_size), int(epochs)
        if tuple(ids.shape) != (N, 2) or int(labels.numel()) != N or (dense is not None and int(np.prod(tuple(dense.shape))) != 0):
            raise ValueError("ids must be [N, 2], dense [N, 0] and labels [N]")
        if N * 2 >= (1 << 31) - 1:
            raise ValueError("N x 2 = %d: the schedule's offsets hold fewer than 2^31 - 1 entries" % (N * 2))
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
        need = int(lib.sprk_train_tower_workspace_bytes(C.byref(ms), N, B, tile))
        if workspace is None:
            workspace = torch.empty(max(need, 16) // 8 + 2, dtype=torch.int64, device=dev)
        c1, c2, eps = adam_constants()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if E and N:
            L.check(lib.sprk_train_tower_fit(C.byref(ms), ptr(ids), ptr(labels), ptr(order_t) if order is not None else None, N, B, tile, E, ptr(t_alpha),
                                             float(c1), float(c2), float(eps), ptr(params), ptr(m), ptr(v), ptr(p), ptr(word), ptr(workspace),
                                             workspace.numel() * workspace.element_size(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
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
    """``CTRModel.fit`` for a ``NeuralCF(arch=2)``: the same arguments (a dict of columns with ``"label"`` or ``y``, or an iterable of ``(features,
    labels)`` batches) and the same return value (per epoch ``[loss, accuracy, roc_auc, pr_auc]``); the trained weights are set on ``model`` and
    Adam's moments kept in ``model._fit_state``, so a second call continues.  This function is the entry: ``NeuralCF(arch=2).fit`` itself still
    raises ``NotImplementedError``, and ``trainer.family_of`` and ``CTRModel.fit`` are as they were."""
    import sys
    fam = family_of(model)
    return model._fit_with(sys.modules[__name__], fam, x, y, batch_size, epochs, learning_rate, order, tile)


# ---------------------------------------------------------------- the towers' vectors

def _flat_view(fam, weights, dev):
    """The flat parameter vector of a weight dict on ``dev``: the dict's own memory where it is the views of one flat vector (a device fit's
    ``TrainResult``), a copy otherwise."""
    import torch
    names, shapes = param_names(fam), param_shapes(fam)
    first = weights[names[0]]
    if all(isinstance(weights[k], torch.Tensor) and weights[k].device == dev and weights[k].dtype == torch.float32 and weights[k].is_contiguous() and
           tuple(weights[k].shape) == shapes[k] for k in names):
        at, together = first.data_ptr(), True
        for k in names:
            together &= weights[k].data_ptr() == at
            at += 4 * int(np.prod(shapes[k]))
        if together:
            return torch.as_strided(first, (n_params(fam),), (1,))
    for k in names:
        if tuple(weights[k].shape) != shapes[k]:
            raise ValueError("weight %r has shape %s, expected %s" % (k, tuple(weights[k].shape), shapes[k]))
    return _flatten(fam, weights, dev)


def default_rows_tile(fam: TowerFamily) -> int:
    tile = ROWS_TILE
    while tile > 1 and rows_lds_bytes(fam, tile) > LDS_BYTES:
        tile //= 2
    return tile


def tower_rows_device(fam: TowerFamily, weights_or_flat, side: str, out=None, tile: Optional[int] = None, device=None):
    """:func:`tower_rows_host` on the device (``sprk_tower_rows``), the same bytes, enqueued on the current stream with no synchronisation.
    ``weights_or_flat``: a weight dict (host arrays or tensors; a device fit's ``TrainResult.weights`` is read where it lies) or the flat
    parameter vector in :func:`param_names` order.  ``out``: a float32 device tensor ``[vocab, >= hidden[-1]]`` with unit column stride whose first
    ``hidden[-1]`` columns are written and whose other floats are left alone; a new ``[vocab, hidden[-1]]`` tensor when None."""
    import ctypes as C

    import torch

    from . import _lib as L
    _check_family(fam)
    if side not in SIDES:
        raise ValueError("side = %r is neither 'item' nor 'user'" % (side,))
    tile = default_rows_tile(fam) if tile is None else int(tile)
    if tile < 1:
        raise ValueError("tile must be >= 1")
    if rows_lds_bytes(fam, tile) > LDS_BYTES:
        raise ValueError("tile = %d needs %d bytes of LDS for this model, more than %d" % (tile, rows_lds_bytes(fam, tile), LDS_BYTES))
    if not torch.cuda.is_available():
        raise RuntimeError("tower_rows_device needs a HIP device: no HIP device is visible (tower_rows_host is the host definition)")
    lib = L.load_library()
    if device is not None:
        dev = torch.device(device)
    elif isinstance(weights_or_flat, torch.Tensor) and weights_or_flat.is_cuda:
        dev = weights_or_flat.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    V, H = fam.columns[SIDES[side]][2], fam.hidden[-1]
    with torch.cuda.device(dev):
        if isinstance(weights_or_flat, torch.Tensor):
            flat = weights_or_flat.detach()
            if flat.device != dev or flat.dtype != torch.float32 or flat.ndim != 1 or not flat.is_contiguous() or int(flat.numel()) != n_params(fam):
                raise ValueError("the flat parameter vector must be a contiguous float32 tensor of %d elements on %s" % (n_params(fam), dev))
        else:
            flat = _flat_view(fam, weights_or_flat, dev)
        if out is None:
            out = torch.empty((V, H), dtype=torch.float32, device=dev)
        if out.dtype != torch.float32 or out.device != dev or out.ndim != 2 or out.shape[0] != V or out.shape[1] < H or (V > 1 and out.stride(0) < H) or \
                out.stride(1) != 1:
            raise ValueError("out must be a float32 [%d, >= %d] tensor on %s with unit column stride" % (V, H, dev))
        ms = _model_struct(fam)
        stride = int(out.stride(0)) if V > 1 else max(int(out.stride(0)), H)
        L.check(lib.sprk_tower_rows(C.byref(ms), C.c_void_p(flat.data_ptr()), SIDES[side], tile, C.c_void_p(out.data_ptr()), stride,
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


class TowerModel(_A.ALSModel):
    """What :func:`towers` returns: an ``als.ALSModel`` whose ``user_factors`` / ``item_factors`` are the trained towers' output vectors, with one
    more attribute: ``sign`` = -1 where the head's kernel is negative and the user vectors are stored negated (largest dot = best score), else 1."""

    def __init__(self, user_factors, item_factors, user_has, item_has, user_count, item_count, sign: int = 1):
        super().__init__(user_factors, item_factors, user_has, item_has, user_count, item_count)
        self.sign = int(sign)


def head_sign(head_kernel) -> int:
    """1 or -1 as ``head/kernel[0, 0]`` is above or below 0; exactly 0 (or NaN) raises: every pair then scores the same."""
    hk = float(np.asarray(_host(head_kernel), dtype=_F).reshape(-1)[0])
    if not (hk > 0 or hk < 0):
        raise ValueError("head/kernel is %r: every pair scores the same, there is nothing to rank by" % hk)
    return 1 if hk > 0 else -1


def _check_topk_width(fam: TowerFamily):
    if fam.hidden[-1] > _A.MAX_RANK:
        raise ValueError("hidden[-1] = %d: sprk_als_topk takes vectors of up to %d elements (tower_rows_device still serves this model)" % (fam.hidden[-1], _A.MAX_RANK))


def _seen_columns(seen):
    if not ("movieId" in seen and "userId" in seen):
        raise KeyError("seen needs the columns 'movieId' and 'userId'")
    return seen["movieId"], seen["userId"]


def towers_host(fam: TowerFamily, w, seen=None):
    """The definition of :func:`towers` on host arrays: ``(user_factors, item_factors, user_has, item_has, user_count, item_count, sign)``, the
    arrays as ``als.als_host`` types them."""
    _check_family(fam)
    _check_topk_width(fam)
    sign = head_sign(w["head/kernel"])
    itf, uf = tower_rows_host(fam, w, "item"), tower_rows_host(fam, w, "user")
    if sign < 0:
        uf = (-uf).astype(_F)
    Vm, Vu = fam.columns[0][2], fam.columns[1][2]
    if seen is None:
        ic, uc = np.zeros(Vm, dtype=np.int32), np.zeros(Vu, dtype=np.int32)
        ih, uh = np.ones(Vm, dtype=np.uint8), np.ones(Vu, dtype=np.uint8)
    else:
        mv, us = (np.asarray(_host(c)).astype(np.int64).reshape(-1) for c in _seen_columns(seen))
        if len(mv) != len(us) or (mv < 0).any() or (mv >= Vm).any() or (us < 0).any() or (us >= Vu).any():
            raise ValueError("seen: movieId and userId must be equally long and inside the vocabularies")
        ic, uc = np.bincount(mv, minlength=Vm).astype(np.int32), np.bincount(us, minlength=Vu).astype(np.int32)
        ih, uh = (ic > 0).astype(np.uint8), (uc > 0).astype(np.uint8)
    return uf, itf, uh, ih, uc, ic, sign


def towers(model_or_result, seen=None, device=None) -> TowerModel:
    """The trained towers as a retrieval model.  ``model_or_result``: a ``NeuralCF(arch=2)`` (its current weights), a ``TrainResult`` of this module
    (a device fit's is read where it lies, no host round trip), or a weight dict.  ``seen``: the training columns, a dict with ``movieId`` and
    ``userId`` (host arrays or device tensors): ``user_count`` / ``item_count`` are the occurrences per id and ``has = count > 0``, so ids the fit
    never saw are neither queries nor candidates; None gives ``has = 1`` and ``count = 0`` everywhere.  A negative ``head/kernel`` stores the user
    vectors negated (exact: every non-zero dot is the exact negation, a dot of ``+0`` stays ``+0``; ``sign = -1``) so that the largest dot stays the
    best score; a zero one raises.  ``hidden[-1]`` above 16, the
    ``sprk_als_topk`` limit, is refused."""
    import torch
    if isinstance(model_or_result, TrainResult):
        w = model_or_result.weights
        fam = family_from_weights(w)
    elif isinstance(model_or_result, dict):
        w = model_or_result
        fam = family_from_weights(w)
    else:
        fam, w = family_of(model_or_result), model_or_result.weights
    _check_family(fam)
    _check_topk_width(fam)
    if not torch.cuda.is_available():
        raise RuntimeError("towers needs a HIP device: no HIP device is visible (towers_host is the host definition)")
    if device is not None:
        dev = torch.device(device)
    elif isinstance(w["head/kernel"], torch.Tensor) and w["head/kernel"].is_cuda:
        dev = w["head/kernel"].device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    Vm, Vu = fam.columns[0][2], fam.columns[1][2]
    with torch.cuda.device(dev):
        flat = _flat_view(fam, w, dev)
        itf, uf = tower_rows_device(fam, flat, "item", device=dev), tower_rows_device(fam, flat, "user", device=dev)
        if seen is None:
            ic, uc = torch.zeros(Vm, dtype=torch.int32, device=dev), torch.zeros(Vu, dtype=torch.int32, device=dev)
            ih, uh = torch.ones(Vm, dtype=torch.uint8, device=dev), torch.ones(Vu, dtype=torch.uint8, device=dev)
        else:
            cols = []
            for c in _seen_columns(seen):
                t = c.detach().to(dev) if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(c).astype(np.int64))).to(dev)
                cols.append(t.to(torch.int64).reshape(-1))
            mv, us = cols
            bad = mv.numel() != us.numel() or (mv.numel() and (int(mv.min()) < 0 or int(mv.max()) >= Vm or int(us.min()) < 0 or int(us.max()) >= Vu))
            if bad:
                raise ValueError("seen: movieId and userId must be equally long and inside the vocabularies")
            ic, uc = torch.bincount(mv, minlength=Vm).to(torch.int32), torch.bincount(us, minlength=Vu).to(torch.int32)
            ih, uh = (ic > 0).to(torch.uint8), (uc > 0).to(torch.uint8)
        sign = head_sign(flat[-2:-1])                                                  # (the one fetch: head/kernel's element)
        if sign < 0:
            uf = -uf
    return TowerModel(uf, itf, uh, ih, uc, ic, sign)
