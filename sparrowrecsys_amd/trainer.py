"""``model.fit`` for the graphs that are "embedding rows + numerics -> Dense/ReLU stack -> one sigmoid": ``NeuralCF(arch=1)`` and
``EmbeddingMLP``, trained with Adam as TensorFlow's ``ApplyAdam`` computes it.

As for ALS and item2vec the project defines its own trainer: :func:`train_host` is the DEFINITION, in numpy with a fixed operation
order, and ``sprk_train_fit`` (csrc/k_train.h, csrc/api_train.h) computes the same bits on the device -- no float atomics, runs that
repeat exactly.  DESIGN.md section 5.12 has the rules and the deviations from Keras; in short:

* everything is float32, every product and every sum rounded on its own (no fused multiply-add), ``sqrt`` and division correctly
  rounded; a Dense unit is ``((0 + x_0 W_0j) + x_1 W_1j + ...) + b_j`` in row order, ReLU is ``z if z > 0 else +0``;
* ``p = sigmoid_def(logit)``: a sigmoid this module states in ``+ - * /`` and exponent manipulation only (no libm call: glibc and the
  device maths library do not round alike);
* step ``b`` takes rows ``[b B, min(N, (b + 1) B))``; an optional ``order`` is applied once, before the first epoch (TensorFlow's
  shuffle buffer is not reproduced);
* parameter gradients are summed in a two-level order: samples of a tile of ``tile`` consecutive samples from ``+0``, then the tiles
  from ``+0``; an embedding row's gradient likewise over the samples that carry its id in that column;
* Adam runs over every element of every parameter on every step (Keras' Adam, not LazyAdam), ``alpha_t`` in doubles on the host;
* ids outside the vocabulary and non-finite numerics or labels are errors, found before the first step (Keras would train on NaN).

The pair-dot ``DeepFM`` is trained under these rules by :mod:`trainer_pair`, whose entry is ``trainer_pair.fit(model, x, ...)``.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Mapping, Optional

import numpy as np

TILE_NARROW, TILE_WIDE, NARROW = 16, 8, 32                          # default_tile(): chosen from the measurement in docs/train_results.md
DEFAULT_BATCH = 4096
MAX_COLS, MAX_LAYERS, MAX_X, MAX_WIDTH = 16, 8, 256, 256
LDS_BYTES = 160 * 1024
BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-7
ERR_ID, ERR_NUMERIC, ERR_LABEL = 1, 2, 3
_F = np.float32

# sigmoid_def's constants (float32): the clamp, log2(e), ln 2 in two parts (the high part has nine significant bits: n * LN2_HI is exact
# for |n| <= 126), the round-to-integer constant 1.5 * 2^23 and Cephes' expf polynomial on [-ln2/2, ln2/2]
SIG_LIMIT = _F(87.0)
SIG_LOG2E = _F(1.44269504088896341)
SIG_LN2_HI = _F(0.693359375)
SIG_LN2_LO = _F(-2.12194440e-4)
SIG_MAGIC = _F(12582912.0)
SIG_POLY = tuple(_F(c) for c in (1.9875691500e-4, 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1))

Family = namedtuple("Family", "columns tables emb_dim xcol xsub n_dense widths layers")
TrainResult = namedtuple("TrainResult", "weights m v step history p")


def _error_message(kind: int, row: int) -> str:
    what = {ERR_ID: "an id outside its column's vocabulary", ERR_NUMERIC: "a numeric feature is not finite", ERR_LABEL: "the label is not finite"}.get(kind)
    return "samples row %d: %s" % (row, what) if what else "error kind %d at %d" % (kind, row)


# ---------------------------------------------------------------- the family

def family_of(model) -> Family:
    """The trainer's view of a model: its id columns ``(name, kind, vocab)`` and their tables, per input row of the first Dense kernel
    the id column it comes from (``xcol``, -1 = a numeric) and the place in the table row or among the numerics (``xsub``), the hidden
    widths and the layer names (the head last).  ``NeuralCF(arch=1)`` and ``EmbeddingMLP`` only."""
    from . import models as M
    if type(model) is M.NeuralCF and model.arch == 1:
        D = model.emb_dim
        xcol, xsub = [0] * D + [1] * D, list(range(D)) * 2                                   # NeuralCF.py:48: movie, then user
    elif type(model) is M.EmbeddingMLP:
        D = model.emb_dim
        rows = model._deep_blocks_order()
        n_x = model._deep_in()
        xcol, xsub = [None] * n_x, [None] * n_x
        for c, k in enumerate(model.EMB_KEYS):
            for d in range(D):
                xcol[rows[k + "_embedding"] + d], xsub[rows[k + "_embedding"] + d] = c, d
        for j, k in enumerate(model.numeric_keys):
            xcol[rows[k]], xsub[rows[k]] = -1, j
    else:
        raise NotImplementedError("fit is implemented for NeuralCF(arch=1) and EmbeddingMLP, and DeepFMv2 through trainer_fm, not for %s%s" %
                                  (type(model).__name__, "(arch=%r)" % model.arch if hasattr(model, "arch") else ""))
    cols = [(c.key, c.kind, int(c.vocab)) for c in model.id_columns]
    fam = Family(cols, ["emb/" + c[0] for c in cols], int(D), xcol, xsub, len(model.numeric_keys), [int(h) for h in model.hidden],
                 ["dense%d" % i for i in range(len(model.hidden))] + ["head"])
    _check_family(fam)
    return fam


def _check_family(fam: Family):
    if not (1 <= len(fam.columns) <= MAX_COLS and 1 <= len(fam.widths) <= MAX_LAYERS and 1 <= len(fam.xcol) <= MAX_X and
            all(1 <= h <= MAX_WIDTH for h in fam.widths) and fam.emb_dim >= 1):
        raise ValueError("the trainer takes up to %d id columns, %d hidden layers of up to %d units and %d input rows" % (MAX_COLS, MAX_LAYERS, MAX_WIDTH, MAX_X))


def param_names(fam: Family):
    """Every trained array, in the order of the device's flat parameter vector."""
    out = list(fam.tables)
    for name in fam.layers:
        out += [name + "/kernel", name + "/bias"]
    return out


def param_shapes(fam: Family):
    s = {t: (c[2], fam.emb_dim) for t, c in zip(fam.tables, fam.columns)}
    fan = len(fam.xcol)
    for name, h in zip(fam.layers, fam.widths + [1]):
        s[name + "/kernel"], s[name + "/bias"] = (fan, h), (h,)
        fan = h
    return s


def default_tile(fam: Family) -> int:
    """The ``tile`` of a fit that names none: 16 where no layer (the input included) is wider than 32, else 8.  A wide stack's tile is
    one workgroup's work and a batch of 4096 has only 128 tiles of 32; a narrow stack's step is short and fewer, larger tiles
    mean fewer partial sums to add (docs/train_results.md has the measurement)."""
    return TILE_NARROW if max([len(fam.xcol)] + list(fam.widths)) <= NARROW else TILE_WIDE


def lds_bytes(fam: Family, tile: int) -> int:
    """The LDS of one workgroup of the forward + backward kernel: the tile's input and activations, and two gradient buffers."""
    wide = max([len(fam.xcol)] + fam.widths)
    return 4 * int(tile) * (len(fam.xcol) + sum(fam.widths) + 2 * wide)


# ---------------------------------------------------------------- the definition

SIG_SPLIT = _F(4097.0)                                             # Dekker's splitter for a 24-bit significand: 2^12 + 1
SIG_CORRECT_N = _F(100.0)                                          # |n| up to which the residual is formed: no product overflows, no part is subnormal


def _split(a):
    c = a * SIG_SPLIT
    hi = c - (c - a)
    return hi, a - hi


def sigmoid_def(z):
    """``1 / (1 + e)``, ``e = exp(t)``, ``t = -z`` clamped to ``[-87, 87]``: ``n`` = ``t log2(e)`` rounded to an integer by adding and
    subtracting ``1.5 * 2^23``, ``r = (t - n LN2_HI) - n LN2_LO``, ``u = (P(r) r) r + r`` with ``P`` in Horner form, so that
    ``e = (1 + u) 2^n`` with the power of two built from its exponent bits; ``p0 = 1 / ((1 + 2^n) + 2^n u)``.  For ``|n| <= 100`` (beyond,
    ``p`` is below 2^-99 or exactly 1) the roundings of that line are taken back: the denominator ``1 + 2^n + 2^n u`` (the product is
    exact) as an exact sum ``dh + dl`` (Knuth's two-sum, twice), the product ``dh p0`` as an exact sum ``x + y`` (Dekker's
    split and product), ``rr = ((1 - x) - y) - dl p0``, ``p = p0 + p0 rr``.  Exactly 0 below ``-87``.  Float32 ``+ - * /`` throughout,
    every operation rounded on its own."""
    z = np.asarray(z, dtype=_F)
    one = _F(1.0)
    with np.errstate(all="ignore"):
        t = np.minimum(np.maximum(-z, -SIG_LIMIT), SIG_LIMIT).astype(_F)
        n = ((t * SIG_LOG2E + SIG_MAGIC) - SIG_MAGIC).astype(_F)
        r = ((t - n * SIG_LN2_HI) - n * SIG_LN2_LO).astype(_F)
        q = np.full_like(r, SIG_POLY[0])
        for c in SIG_POLY[1:]:
            q = q * r + c
        u = ((q * r) * r + r).astype(_F)
        scale = ((np.where(n == n, n, 0).astype(np.int32) + np.int32(127)) << np.int32(23)).view(_F)
        a, b = one + scale, scale * u
        aa = a - one
        al = (one - (a - aa)) + (scale - aa)
        dh = a + b
        bb = dh - a
        dl = ((a - (dh - bb)) + (b - bb)) + al
        p0 = one / dh
        x = dh * p0
        (h1, l1), (h2, l2) = _split(dh), _split(p0)
        y = ((h1 * h2 - x) + h1 * l2 + l1 * h2) + l1 * l2
        rr = ((one - x) - y) - dl * p0
        p = np.where(np.abs(n) <= SIG_CORRECT_N, p0 + p0 * rr, p0).astype(_F)
        return np.where(z < -SIG_LIMIT, _F(0.0), p).astype(_F)


def _dense(x, W, b):
    z = np.zeros((x.shape[0], W.shape[1]), dtype=_F)
    for k in range(W.shape[0]):
        z = z + x[:, k:k + 1] * W[k][None, :]
    return z + b[None, :]


def _back(W, dz):
    da = np.zeros((dz.shape[0], W.shape[0]), dtype=_F)
    for j in range(W.shape[1]):
        da = da + W[:, j][None, :] * dz[:, j:j + 1]
    return da


def _tiles(a, tile):
    n = a.shape[0]
    T = (n + tile - 1) // tile
    pad = np.zeros((T * tile,) + a.shape[1:], dtype=_F)                # (a zero row adds +0: no bit changes)
    pad[:n] = a
    return pad.reshape((T, tile) + a.shape[1:])


def _sum_tiles(s):
    total = np.zeros(s.shape[1:], dtype=_F)
    for t in range(s.shape[0]):
        total = total + s[t]
    return total


def _grad_kernel(a, dz, tile):
    A, Z = _tiles(a, tile), _tiles(dz, tile)
    s = np.zeros((A.shape[0], a.shape[1], dz.shape[1]), dtype=_F)
    for i in range(tile):
        s = s + A[:, i, :, None] * Z[:, i, None, :]
    return _sum_tiles(s)


def _grad_bias(dz, tile):
    Z = _tiles(dz, tile)
    s = np.zeros((Z.shape[0], dz.shape[1]), dtype=_F)
    for i in range(tile):
        s = s + Z[:, i]
    return _sum_tiles(s)


def _grad_table(idc, dxc, vocab, tile):
    n = len(idc)
    g = np.zeros((vocab, dxc.shape[1]), dtype=_F)
    uniq, inv = np.unique(idc[idc >= 0], return_inverse=True)
    if not len(uniq):
        return g
    slot = np.full(n, -1, dtype=np.int64)
    slot[idc >= 0] = inv
    T = (n + tile - 1) // tile
    s = np.zeros((T, len(uniq), dxc.shape[1]), dtype=_F)
    for i in range(tile):
        rows = np.arange(T) * tile + i
        keep = rows < n
        keep[keep] = slot[rows[keep]] >= 0
        t, r = np.flatnonzero(keep), rows[keep]
        s[t, slot[r]] = s[t, slot[r]] + dxc[r]                         # (one sample per tile: the pairs are distinct)
    g[uniq] = _sum_tiles(s)
    return g


def input_rows(fam: Family, w: Mapping[str, np.ndarray], ids, dense):
    """``x [n, n_x]``: per input row the table row's element (zeros for id -1) or the numeric."""
    x = np.zeros((ids.shape[0], len(fam.xcol)), dtype=_F)
    for k, (c, s) in enumerate(zip(fam.xcol, fam.xsub)):
        if c < 0:
            x[:, k] = dense[:, s]
        else:
            x[:, k] = np.where(ids[:, c] >= 0, w[fam.tables[c]][np.maximum(ids[:, c], 0), s], _F(0.0))
    return x


def forward_host(fam: Family, w, ids, dense, keep=None):
    """The definition's probabilities ``[n]`` for packed rows; ``keep`` (a list) receives the input and every activation."""
    a = input_rows(fam, w, ids, dense)
    acts = [a]
    with np.errstate(all="ignore"):
        for name in fam.layers[:-1]:
            z = _dense(a, w[name + "/kernel"], w[name + "/bias"])
            a = np.where(z > 0, z, _F(0.0)).astype(_F)
            acts.append(a)
        logit = _dense(a, w["head/kernel"], w["head/bias"])[:, 0]
    if keep is not None:
        keep.extend(acts)
    return sigmoid_def(logit)


def step_gradients(fam: Family, w, ids, dense, labels, tile: Optional[int] = None):
    """One step's gradients: ``({name: gradient}, p)`` for the batch ``(ids, dense, labels)`` under the weights ``w``."""
    ids, dense, labels = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F), np.asarray(labels, dtype=_F)
    n, tile = ids.shape[0], default_tile(fam) if tile is None else int(tile)
    acts = []
    p = forward_host(fam, w, ids, dense, acts)
    g = {}
    with np.errstate(all="ignore"):
        dz = ((p - labels) / _F(n)).astype(_F)[:, None]
        for li in range(len(fam.layers) - 1, -1, -1):
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


def adam_alpha(lr: float, t: int) -> np.float32:
    """``float32(lr sqrt(1 - beta2^t) / (1 - beta1^t))`` in doubles (ApplyAdam's ``lr_t``)."""
    return _F(float(lr) * math.sqrt(1.0 - BETA2 ** int(t)) / (1.0 - BETA1 ** int(t)))


def adam_constants():
    """``(1 - beta1, 1 - beta2, epsilon)`` as the float32 values both implementations use."""
    return _F(1.0) - _F(BETA1), _F(1.0) - _F(BETA2), _F(EPSILON)


def adam_step(w, m, v, g, alpha):
    """``m += (g - m)(1 - beta1)``, ``v += (g g - v)(1 - beta2)``, ``w -= alpha m / (sqrt(v) + epsilon)``, in place, float32."""
    c1, c2, eps = adam_constants()
    with np.errstate(all="ignore"):
        m += (g - m) * c1
        v += (g * g - v) * c2
        w -= (_F(alpha) * m) / (np.sqrt(v) + eps)


def _check_args(batch_size, epochs, learning_rate, tile):
    if int(batch_size) < 1 or int(tile) < 1:
        raise ValueError("batch_size and tile must be >= 1")
    if int(epochs) < 0:
        raise ValueError("epochs = %r is negative" % (epochs,))
    if not (np.isfinite(learning_rate) and learning_rate > 0):
        raise ValueError("learning_rate = %r must be finite and > 0" % (learning_rate,))


def validate_host(fam: Family, ids, dense, labels):
    """The checks before the first step: the smallest ``(kind, row)`` raises ``ValueError``."""
    kind = np.zeros(ids.shape[0], dtype=np.int64)
    kind[~np.isfinite(labels)] = ERR_LABEL
    if dense.shape[1]:
        kind[~np.isfinite(dense).all(axis=1)] = ERR_NUMERIC
    bad = np.zeros(ids.shape[0], dtype=bool)
    for c, (_, k, vocab) in enumerate(fam.columns):
        bad |= (ids[:, c] < (-1 if k == "genre" else 0)) | (ids[:, c] >= vocab)
    kind[bad] = ERR_ID
    if kind.any():
        key = int(((kind[kind != 0] << 32) | np.flatnonzero(kind)).min())
        raise ValueError(_error_message(key >> 32, key & 0xffffffff))


def _check_order(order, n):
    order = np.asarray(order).astype(np.int64).reshape(-1)
    if len(order) != n or not np.array_equal(np.sort(order), np.arange(n)):
        raise ValueError("order must be a permutation of 0 .. N - 1")
    return order


def _copy_state(fam, weights, state):
    names, shapes = param_names(fam), param_shapes(fam)
    w = {}
    for k in names:
        a = np.array(weights[k].detach().cpu().numpy() if hasattr(weights[k], "detach") else weights[k], dtype=_F)
        if a.shape != shapes[k]:
            raise ValueError("weight %r has shape %s, expected %s" % (k, a.shape, shapes[k]))
        w[k] = a
    if state is None:
        return w, {k: np.zeros_like(w[k]) for k in names}, {k: np.zeros_like(w[k]) for k in names}, 0
    m, v, step = state
    return w, {k: np.array(m[k], dtype=_F) for k in names}, {k: np.array(v[k], dtype=_F) for k in names}, int(step)


def train_host(fam: Family, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
               order=None, tile: Optional[int] = None, state=None) -> TrainResult:
    """The definition (module docstring) on packed host arrays: ``ids [N, C]`` int32 in ``model.id_columns``
    order, ``dense [N, F]`` float32 in ``numeric_keys`` order, ``labels [N]`` float32.  ``state = (m, v, step)`` continues an earlier
    fit.  -> ``TrainResult``: the trained weights, ``m``, ``v`` (dicts like the weights), the step count, per epoch ``[loss, accuracy,
    roc_auc, pr_auc]`` of the training forward's own probabilities (``metrics.evaluate_scores``) and the last epoch's ``p [N]`` in step
    order.  Nothing is changed when a check fails."""
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
    s = L.TrainModel()
    s.n_cols, s.n_dense, s.emb_dim, s.n_x, s.n_layers = len(fam.columns), fam.n_dense, fam.emb_dim, len(fam.xcol), len(fam.widths)
    for c, (_, kind, vocab) in enumerate(fam.columns):
        s.vocab[c], s.genre[c] = vocab, 1 if kind == "genre" else 0
    for i, h in enumerate(fam.widths):
        s.width[i] = h
    for k, (c, x) in enumerate(zip(fam.xcol, fam.xsub)):
        s.xcol[k], s.xsub[k] = c, x
    return s


def train_device(fam: Family, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
                 order=None, tile: Optional[int] = None, state=None, device=None, workspace=None, num_thresholds: int = 200) -> TrainResult:
    """:func:`train_host` on the device (``sprk_train_fit``): the same bits in every weight, ``m``, ``v`` and ``p``; the history through
    ``metrics.DeviceMetrics`` (accuracy and both AUCs bit for bit, the loss within a float64 sum's rounding).  ``ids`` / ``dense`` /
    ``labels`` / ``order`` are host arrays or device tensors; tensors on the device are used where they are.  The whole fit is
    enqueued on the current stream; the one synchronisation fetches the error word.  -> ``TrainResult`` of device tensors (views of
    three flat vectors)."""
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

    def up(a, dt):
        if hasattr(a, "detach"):
            return a.detach().to(dev).to(dt).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.float32: _F}[dt])).to(dev)
    with torch.cuda.device(dev):
        ids, labels = up(ids, torch.int32), up(labels, torch.float32).reshape(-1)
        N, B, E = int(ids.shape[0]), int(batch_size), int(epochs)
        dense = up(dense, torch.float32).reshape(N, fam.n_dense)
        if tuple(ids.shape) != (N, len(fam.columns)) or int(labels.numel()) != N:
            raise ValueError("ids must be [N, %d], dense [N, %d] and labels [N]" % (len(fam.columns), fam.n_dense))
        if N * len(fam.columns) >= (1 << 31) - 1:
            raise ValueError("N x id columns = %d: the schedule's offsets hold fewer than 2^31 - 1 entries" % (N * len(fam.columns)))
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
        names = param_names(fam)
        shapes = param_shapes(fam)
        for k in names:
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
        need = int(lib.sprk_train_workspace_bytes(C.byref(ms), N, B, tile))
        if workspace is None:
            workspace = torch.empty(max(need, 16) // 8 + 2, dtype=torch.int64, device=dev)
        c1, c2, eps = adam_constants()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if E and N:
            L.check(lib.sprk_train_fit(C.byref(ms), ptr(ids), ptr(dense) if fam.n_dense else None, ptr(labels), ptr(order_t) if order is not None else None,
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
