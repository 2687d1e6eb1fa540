"""``trainer_pair.fit(model, ...)`` for ``DeepFM`` -- the reference's ``DeepFM.py`` graph: first-order weights that are rows of the head's
kernel, ``P`` explicit pairwise dots of FM table rows, a deep stack over deep-only tables (or the FM tables, ``share_deep_tables=True``)
and the numerics, one sigmoid -- trained with Adam under the rules of :mod:`trainer` (DESIGN.md sections 5.12 and 5.21).

:func:`train_host` is the DEFINITION, in numpy with a fixed operation order; ``sprk_train_pair_fit`` (csrc/k_train_pair.h,
csrc/api_train_pair.h) computes the same bits on the device.  The arithmetic is the trainer's own, through the trainer's own functions:
float32, every product and sum rounded on its own, no fused multiply-add, sums from ``+0`` in index order, ReLU ``z if z > 0 else +0``,
``sigmoid_def``, the two-level gradient sums (a tile's samples, then the tiles), Adam over every element of every array on every step,
``alpha_t`` in doubles on the host, ``order`` applied once; non-finite inputs and ids outside the vocabulary are errors found before the
first step.  What this graph adds (``F`` fields, ``D = emb_dim``, ``P`` pairs, ``H = hidden[-1]``, ``T = fo_total``; ``ids [N, F]`` in
``model.fields`` order):

* ``e_f`` = row ``id`` of ``emb/<key f>``, zeros for id -1 (genre kinds): such a field adds no first-order term and has no schedule entry;
* the deep input: per row of ``deep0/kernel`` (name-sorted: ``model._deep_rows()``) one element of the deep table's row -- ``deep_emb/<key>``,
  or ``emb/<key>`` when ``shared`` -- or a numeric; the ``deep{i}`` layers as ``trainer._dense`` + ReLU up to the last activation ``a``;
* ``dot_p = ((+0 + e_a[0] e_b[0]) + e_a[1] e_b[1]) + ...`` in element order, for the pairs ``(a, b)`` in ``model.pairs`` order;
* the logit is one Dense unit over the head's inputs in ``head/kernel`` row order: from ``+0`` the first-order rows ``head/kernel[fo_off_f +
  id_f]`` of the fields in ascending ``fo_off`` (their product with 1 is exact; only the rows a sample carries are added), then ``dot_p
  head/kernel[T + p]`` in pair order, then ``a_j head/kernel[T + P + j]``, then ``head/bias``;
* backwards ``g = (p - y) / n``; ``head/kernel[:T]`` is a table of width 1 over ``g``, ``head/kernel[T:]`` a Dense kernel over ``[dots, a]``;
  ``t_p = +0 + head/kernel[T + p] g``; the deep stack as ``trainer.step_gradients``, down to the deep input's gradient ``dx``;
* per sample a field's FM-row gradient starts at ``+0``; the pairs are walked in pair order, for pair ``p``: first ``de[a] += t_p e_b``, then
  ``de[b] += t_p e_a`` (each ``e`` the forward's value; a pair ``(a, a)`` adds the same vector twice); with ``shared`` the deep input's gradient
  for that key is added after all pairs, without it that gradient is ``deep_emb/<key>``'s;
* one run of samples per ``(field, id)`` and batch serves three rows: ``emb/<key>[id]``, ``deep_emb/<key>[id]`` and ``head/kernel[fo_off + id]``;
  rows and Dense parameters are summed within a tile from ``+0``, then over the tiles from ``+0``; a row without a run gets ``g = +0``;
* a NaN that reaches a stored value (``p``, a weight, ``m``, ``v``) is stored as the quiet NaN ``0x7fc00000``, as in :mod:`trainer_fm`.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np

from . import trainer as _T
from .trainer import (DEFAULT_BATCH, LDS_BYTES, TrainResult, _back, _check_args, _check_order, _dense, _error_message, _grad_bias, _grad_kernel, _grad_table,
                      adam_alpha, adam_constants, sigmoid_def)
from .trainer_fm import QNAN, _canonical, _rows, adam_step_fm

MAX_FIELDS, MAX_PAIRS, MAX_LAYERS, MAX_WIDTH, MAX_X, MAX_DIM = 8, 32, 8, 256, 256, 64
DEFAULT_TILE = 8                                                      # chosen from the tile sweep in docs/train_pair_results.md
MAX_ROWS = (1 << 31) - 1                                              # the schedule's key holds a row in 32 bits
_F = np.float32


class PairFamily(namedtuple("PairFamily", "fields fo_off fo_total pairs deep_cols shared emb_dim n_dense hidden xsrc xsub")):
    """``fields``: ``(key, kind, vocab)`` in ``model.fields`` order (the id columns of ``pack_device``); ``fo_off``: per field its first row
    in ``head/kernel``, ``fo_total`` those rows' count; ``pairs``: ``(field index a, field index b)`` in ``model.pairs`` order; ``deep_cols``:
    the field indices of ``model.deep_emb``; ``shared``: the deep part reads ``emb/<key>``; per row of ``deep0/kernel`` ``xsrc`` = the place in
    ``deep_cols`` of the table it comes from (-1 = a numeric) and ``xsub`` = the element of the table row or the numeric's index."""
    __slots__ = ()

    @property
    def columns(self):
        return self.fields


def make_family(fields, pairs, deep_emb, shared, emb_dim, hidden, numeric_keys) -> PairFamily:
    """The family of a field list (``(key, kind, vocab)``), a pair list and a deep key list by key, as ``models.DeepFM`` lays them out."""
    from . import models as M
    fields = [(k, kind, int(v)) for k, kind, v in fields]
    keys = [k for k, _, _ in fields]
    if len(set(keys)) != len(keys) or any(k not in keys for ab in pairs for k in ab) or any(k not in keys for k in deep_emb):
        raise ValueError("the fields' keys must be distinct and every pair and deep key must name a field")
    fo = M.first_order_offsets(fields)
    D = int(emb_dim)
    names = sorted([k + "_embedding" for k in deep_emb] + list(numeric_keys))
    xsrc, xsub = [], []
    for name in names:                                                 # models.DeepFM._deep_rows(): name-sorted blocks
        if name in numeric_keys:
            xsrc.append(-1)
            xsub.append(list(numeric_keys).index(name))
        else:
            xsrc += [list(deep_emb).index(name[:-len("_embedding")])] * D
            xsub += list(range(D))
    fam = PairFamily(fields, [int(fo[k]) for k in keys], int(fo["__total__"]), [(keys.index(a), keys.index(b)) for a, b in pairs],
                     [keys.index(k) for k in deep_emb], bool(shared), D, len(numeric_keys), [int(h) for h in hidden], xsrc, xsub)
    _check_family(fam)
    return fam


def family_of(model) -> PairFamily:
    """The trainer's view of a ``DeepFM`` (that class itself: a subclass may compute another graph)."""
    from . import models as M
    if type(model) is not M.DeepFM:
        raise NotImplementedError("trainer_pair trains DeepFM, not %s" % type(model).__name__)
    fam = make_family(model.fields, model.pairs, model.deep_emb, model.share_deep_tables, model.emb_dim, model.hidden, list(model.numeric_keys))
    rows, n_x = model._deep_rows()
    assert n_x == len(fam.xsrc) and all(fam.xsrc[rows[k]] == -1 for k in model.numeric_keys)
    return fam


def _check_family(fam: PairFamily):
    F, n_x = len(fam.fields), len(fam.xsrc)
    ok = (1 <= F <= MAX_FIELDS and 1 <= len(fam.pairs) <= MAX_PAIRS and 1 <= len(fam.hidden) <= MAX_LAYERS and all(1 <= h <= MAX_WIDTH for h in fam.hidden) and
          1 <= n_x <= MAX_X and 1 <= fam.emb_dim <= MAX_DIM and fam.n_dense >= 0 and all(v >= 1 for _, _, v in fam.fields))
    if not ok:
        raise ValueError("trainer_pair takes up to %d fields, 1 to %d pairs, up to %d hidden layers of up to %d units, 1 to %d deep inputs and emb_dim up to %d" %
                         (MAX_FIELDS, MAX_PAIRS, MAX_LAYERS, MAX_WIDTH, MAX_X, MAX_DIM))
    if any(not (0 <= a < F and 0 <= b < F) for a, b in fam.pairs) or len(set(fam.deep_cols)) != len(fam.deep_cols) or any(not 0 <= c < F for c in fam.deep_cols):
        raise ValueError("a pair names two fields (the same one twice is legal) and the deep keys are distinct fields")
    want = sorted([(j, d) for j in range(len(fam.deep_cols)) for d in range(fam.emb_dim)] + [(-1, j) for j in range(fam.n_dense)])
    if sorted(zip(fam.xsrc, fam.xsub)) != want:
        raise ValueError("the rows of deep0/kernel are every element of every deep table's row and every numeric, once each")
    if sum(v for _, _, v in fam.fields) >= MAX_ROWS:
        raise ValueError("the fields' %d rows: the schedule's key holds fewer than 2^31 - 1 rows" % sum(v for _, _, v in fam.fields))


def param_names(fam: PairFamily):
    """Every trained array -- all of ``DeepFM.weight_shapes()`` -- in the order of the device's flat parameter vector: ``emb/<key>`` in field
    order, ``deep_emb/<key>`` in ``deep_emb`` order (absent when shared), the deep layers' kernels and biases, ``head/bias``, then
    ``head/kernel``: its first ``fo_total`` rows, trained like a table of width 1, sit next to its Dense tail ``[P + H]``."""
    out = ["emb/" + k for k, _, _ in fam.fields]
    if not fam.shared:
        out += ["deep_emb/" + fam.fields[c][0] for c in fam.deep_cols]
    for i in range(len(fam.hidden)):
        out += ["deep%d/kernel" % i, "deep%d/bias" % i]
    return out + ["head/bias", "head/kernel"]


def param_shapes(fam: PairFamily):
    s = {"emb/" + k: (v, fam.emb_dim) for k, _, v in fam.fields}
    if not fam.shared:
        s.update({"deep_emb/" + fam.fields[c][0]: (fam.fields[c][2], fam.emb_dim) for c in fam.deep_cols})
    fan = len(fam.xsrc)
    for i, h in enumerate(fam.hidden):
        s["deep%d/kernel" % i], s["deep%d/bias" % i] = (fan, h), (h,)
        fan = h
    s["head/kernel"], s["head/bias"] = (fam.fo_total + len(fam.pairs) + fam.hidden[-1], 1), (1,)
    return s


def default_tile(fam: PairFamily) -> int:
    """The ``tile`` of a fit that names none: 8, halved until the tile fits the LDS -- the tile sweep of docs/train_pair_results.md at batch
    4096: the reference shape 318 us a step at tile 2, 248 at 4, 237 at 8, 248 at 16, 331 at 32; config 2's 434, 358, 351, 369, 469."""
    tile = DEFAULT_TILE
    while tile > 1 and lds_bytes(fam, tile) > LDS_BYTES:
        tile //= 2
    return tile


def _wide(fam: PairFamily) -> int:
    return max([len(fam.xsrc)] + list(fam.hidden))


def lds_bytes(fam: PairFamily, tile: int) -> int:
    """The LDS of one workgroup of the step kernel, per sample of the tile: the fields' FM rows, the deep inputs, the activations, the dots,
    their gradients ``t`` and two gradient buffers."""
    per = len(fam.fields) * fam.emb_dim + len(fam.xsrc) + sum(fam.hidden) + 2 * len(fam.pairs) + 2 * _wide(fam)
    return 4 * int(tile) * per


# ---------------------------------------------------------------- the definition

def _deep_table(fam: PairFamily, j: int) -> str:
    return ("emb/" if fam.shared else "deep_emb/") + fam.fields[fam.deep_cols[j]][0]


def _deep_rows_of(fam: PairFamily, j: int):
    """The rows of ``deep0/kernel`` that read deep table ``j``, in element order."""
    ks = [k for k in range(len(fam.xsrc)) if fam.xsrc[k] == j]
    ks.sort(key=lambda k: fam.xsub[k])
    return ks


def forward_host(fam: PairFamily, w, ids, dense, keep: Optional[dict] = None):
    """The definition's probabilities ``[n]`` for packed rows; ``keep`` (a dict) receives every intermediate the backward pass reads."""
    ids, dense = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, D, T, P = ids.shape[0], fam.emb_dim, fam.fo_total, len(fam.pairs)
    hk = w["head/kernel"]
    with np.errstate(all="ignore"):
        e = [_rows(w, "emb/" + k, ids[:, f], D) for f, (k, _, _) in enumerate(fam.fields)]
        rows = [_rows(w, _deep_table(fam, j), ids[:, c], D) for j, c in enumerate(fam.deep_cols)]
        x = np.zeros((n, len(fam.xsrc)), dtype=_F)
        for k, (j, s) in enumerate(zip(fam.xsrc, fam.xsub)):
            x[:, k] = dense[:, s] if j < 0 else rows[j][:, s]
        a = x
        acts = [a]
        for i in range(len(fam.hidden)):
            z = _dense(a, w["deep%d/kernel" % i], w["deep%d/bias" % i])
            a = np.where(z > 0, z, _F(0.0)).astype(_F)
            acts.append(a)
        dots = np.zeros((n, P), dtype=_F)
        for p, (fa, fb) in enumerate(fam.pairs):
            s = np.zeros(n, dtype=_F)
            for d in range(D):
                s = s + e[fa][:, d] * e[fb][:, d]
            dots[:, p] = s
        z = np.zeros(n, dtype=_F)
        for f in sorted(range(len(fam.fields)), key=lambda f: fam.fo_off[f]):
            have = ids[:, f] >= 0
            z = np.where(have, z + hk[fam.fo_off[f] + np.maximum(ids[:, f], 0), 0], z).astype(_F)
        cat = np.concatenate([dots, a], axis=1).astype(_F)
        for k in range(cat.shape[1]):
            z = z + cat[:, k] * hk[T + k, 0]
        logit = (z + w["head/bias"][0]).astype(_F)
        p = sigmoid_def(logit)
    if keep is not None:
        keep.update(e=e, acts=acts, cat=cat, logit=logit)
    return _canonical(p)


def step_gradients(fam: PairFamily, w, ids, dense, labels, tile: Optional[int] = None):
    """One step's gradients: ``({name: gradient}, p)`` for the batch ``(ids, dense, labels)`` under the weights ``w``."""
    ids, labels = np.asarray(ids, dtype=np.int32), np.asarray(labels, dtype=_F)
    dense = np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, tile = ids.shape[0], default_tile(fam) if tile is None else int(tile)
    T, P, L = fam.fo_total, len(fam.pairs), len(fam.hidden)
    k_ = {}
    p = forward_host(fam, w, ids, dense, k_)
    e, acts = k_["e"], k_["acts"]
    g = {}
    with np.errstate(all="ignore"):
        dl = ((p - labels) / _F(n)).astype(_F)[:, None]
        head = np.zeros((T + P + fam.hidden[-1], 1), dtype=_F)
        for f, (_, _, vocab) in enumerate(fam.fields):
            head[fam.fo_off[f]:fam.fo_off[f] + vocab] = _grad_table(ids[:, f], dl, vocab, tile)
        head[T:] = _grad_kernel(k_["cat"], dl, tile)
        g["head/kernel"], g["head/bias"] = head, _grad_bias(dl, tile)
        da = _back(w["head/kernel"][T:], dl)
        t = da[:, :P]
        dz = np.where(acts[L] > 0, da[:, P:], _F(0.0)).astype(_F)
        for i in range(L - 1, -1, -1):
            a = acts[i]
            g["deep%d/kernel" % i], g["deep%d/bias" % i] = _grad_kernel(a, dz, tile), _grad_bias(dz, tile)
            da = _back(w["deep%d/kernel" % i], dz)
            dz = np.where(a > 0, da, _F(0.0)).astype(_F) if i else da
        de = [np.zeros((n, fam.emb_dim), dtype=_F) for _ in fam.fields]
        for q, (fa, fb) in enumerate(fam.pairs):
            tq = t[:, q:q + 1]
            de[fa] = de[fa] + tq * e[fb]
            de[fb] = de[fb] + tq * e[fa]
        for j, c in enumerate(fam.deep_cols):
            dx = dz[:, _deep_rows_of(fam, j)]
            if fam.shared:
                de[c] = de[c] + dx
            else:
                g[_deep_table(fam, j)] = _grad_table(ids[:, c], dx, fam.fields[c][2], tile)
        for f, (k, _, vocab) in enumerate(fam.fields):
            g["emb/" + k] = _grad_table(ids[:, f], de[f], vocab, tile)
    return g, p


def validate_host(fam: PairFamily, ids, dense, labels):
    """The trainer's checks before the first step, with its messages."""
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


def train_host(fam: PairFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
               order=None, tile: Optional[int] = None, state=None) -> TrainResult:
    """The definition on packed host arrays, with ``trainer.train_host``'s arguments and returns: ``ids [N, fields]`` int32 in
    ``model.fields`` order, ``dense [N, n_dense]`` float32, ``labels [N]`` float32; ``order`` a permutation of the rows, applied once;
    ``state = (m, v, step)`` continues an earlier fit.  Nothing is changed when a check fails."""
    from .metrics import evaluate_scores
    tile = default_tile(fam) if tile is None else int(tile)
    _check_args(batch_size, epochs, learning_rate, tile)
    ids, dense, labels = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F), np.asarray(labels, dtype=_F).reshape(-1)
    N, B = ids.shape[0], int(batch_size)
    dense = dense.reshape(N, fam.n_dense)
    if ids.shape != (N, len(fam.fields)) or labels.shape != (N,):
        raise ValueError("ids must be [N, %d], dense [N, %d] and labels [N]" % (len(fam.fields), fam.n_dense))
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
                adam_step_fm(w[k], m[k], v[k], g[k], alpha)
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
    s = L.TrainPairModel()
    s.n_fields, s.n_dense, s.emb_dim, s.n_pairs, s.n_deep, s.shared = len(fam.fields), fam.n_dense, fam.emb_dim, len(fam.pairs), len(fam.deep_cols), int(fam.shared)
    s.n_x, s.n_layers = len(fam.xsrc), len(fam.hidden)
    for c, (_, kind, vocab) in enumerate(fam.fields):
        s.vocab[c], s.genre[c], s.fo_off[c] = vocab, 1 if kind == "genre" else 0, fam.fo_off[c]
    for q, (a, b) in enumerate(fam.pairs):
        s.pair_a[q], s.pair_b[q] = a, b
    for j, c in enumerate(fam.deep_cols):
        s.deep_col[j] = c
    for i, h in enumerate(fam.hidden):
        s.width[i] = h
    for k, (j, x) in enumerate(zip(fam.xsrc, fam.xsub)):
        s.xsrc[k], s.xsub[k] = j, x
    return s


def train_device(fam: PairFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
                 order=None, tile: Optional[int] = None, state=None, device=None, workspace=None, num_thresholds: int = 200) -> TrainResult:
    """:func:`train_host` on the device (``sprk_train_pair_fit``): the same bits in every weight, ``m``, ``v`` and ``p``; the history through
    ``metrics.DeviceMetrics`` (accuracy and both AUCs bit for bit, the loss within a float64 sum's rounding).  Arguments and returns are
    ``trainer.train_device``'s; the whole fit is enqueued on the current stream and the one synchronisation fetches the error word."""
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
    n_f = len(fam.fields)

    def up(a, dt):
        if hasattr(a, "detach"):
            return a.detach().to(dev).to(dt).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.float32: _F}[dt])).to(dev)
    with torch.cuda.device(dev):
        ids, labels = up(ids, torch.int32), up(labels, torch.float32).reshape(-1)
        N, B, E = int(ids.shape[0]), int(batch_size), int(epochs)
        dense = up(dense, torch.float32).reshape(N, fam.n_dense)
        if tuple(ids.shape) != (N, n_f) or int(labels.numel()) != N:
            raise ValueError("ids must be [N, %d], dense [N, %d] and labels [N]" % (n_f, fam.n_dense))
        if N * n_f >= (1 << 31) - 1:
            raise ValueError("N x fields = %d: the schedule's offsets hold fewer than 2^31 - 1 entries" % (N * n_f))
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
        need = int(lib.sprk_train_pair_workspace_bytes(C.byref(ms), N, B, tile))
        if workspace is None:
            workspace = torch.empty(max(need, 16) // 8 + 2, dtype=torch.int64, device=dev)
        c1, c2, eps = adam_constants()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if E and N:
            L.check(lib.sprk_train_pair_fit(C.byref(ms), ptr(ids), ptr(dense) if fam.n_dense else None, ptr(labels), ptr(order_t) if order is not None else None,
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
    """``CTRModel.fit`` for a ``DeepFM``: the same arguments (a dict of columns with ``"label"`` or ``y``, or an iterable of ``(features,
    labels)`` batches) and the same return value (per epoch ``[loss, accuracy, roc_auc, pr_auc]``); the trained weights are set on
    ``model`` and Adam's moments kept in ``model._fit_state``, so a second call continues.  This function is the entry: ``DeepFM.fit``
    itself still raises ``NotImplementedError``, and ``trainer.family_of`` and ``CTRModel.fit`` are as they were."""
    import sys
    fam = family_of(model)
    return model._fit_with(sys.modules[__name__], fam, x, y, batch_size, epochs, learning_rate, order, tile)
