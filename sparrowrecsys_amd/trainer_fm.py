"""``model.fit`` for ``DeepFMv2`` -- first order + sum-of-squares FM cross over per-field Dense projections + a deep stack, one sigmoid --
trained with Adam under the rules of :mod:`trainer` (DESIGN.md sections 5.12 and 5.13).

:func:`train_host` is the DEFINITION, in numpy with a fixed operation order; ``sprk_train_fm_fit`` (csrc/k_train_fm.h,
csrc/api_train_fm.h) computes the same bits on the device.  The arithmetic is the trainer's own, through the trainer's own functions:
float32, every product and sum rounded on its own, sums from ``+0`` in index order, ReLU ``z if z > 0 else +0``, ``sigmoid_def``, the
two-level gradient sums (a tile's samples, then the tiles), Adam over every element on every step.  What this graph adds
(``G = len(order) + 1`` groups, ``P = proj_dim``):

* ``fo_cat`` = the ``fo_cat/kernel`` rows of the fields' ids added in ascending offset order from ``+0`` (id -1 adds nothing), then
  ``+ fo_cat/bias``; ``fo_num = _dense(numerics, fo_num)``; ``first = fo_cat + fo_num``;
* ``v_g = _dense(e_g, proj/order[g])`` for ``g < G - 1`` (``e_g`` the table row, zeros for id -1), ``v_{G-1} = _dense(numerics, proj/num)``;
* ``s_j = sum_g v_gj`` and ``q_j = sum_g v_gj v_gj`` in group order from ``+0``; ``fm_j = s_j s_j - q_j``;
* the ``v_g`` in group order feed the ``deep{i}`` stack; ``logit = _dense([first, fm, deep], head)``;
* backwards ``dv_gj = d_flat_gj + d_fm_j (2 (s_j - v_gj))``: the difference, its double, the product, the sum, in that order;
* ``fo_cat/kernel`` is a table of width 1 over ``d_first``: one run of samples per ``(field, id)`` serves it and the ``emb/`` row;
* a field outside ``order`` keeps its ``emb/`` table in the parameter vector with gradient 0 (Adam from zero moments leaves it as it is);
* a NaN that reaches a stored value (``p``, a weight, ``m``, ``v``) is stored as the quiet NaN ``0x7fc00000``: processors do not agree
  on the sign of a NaN they generate, and IEEE 754 leaves it open.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np

from . import trainer as _T
from .trainer import (DEFAULT_BATCH, LDS_BYTES, TrainResult, _back, _check_args, _check_order, _dense, _error_message, _grad_bias, _grad_kernel, _grad_table,
                      adam_alpha, adam_constants, adam_step, sigmoid_def)

MAX_FIELDS, MAX_PROJ, MAX_FLAT, MAX_WIDTH, MAX_LAYERS, MAX_IN = 8, 128, 1024, 256, 8, 256
DEFAULT_TILE = 8                                                      # chosen from the tile sweep in docs/train_fm_results.md
_F = np.float32
QNAN = np.array([0x7fc00000], dtype=np.uint32).view(_F)[0]


class FMFamily(namedtuple("FMFamily", "fields fo_off order emb_dim proj_dim hidden n_dense")):
    """``fields``: ``(key, kind, vocab)`` in ``model.id_columns`` order; ``fo_off``: per field its first row in ``fo_cat/kernel``;
    ``order``: the field keys of groups ``0 .. G - 2``; ``n_dense``: the numerics, in ``numeric_keys`` order."""
    __slots__ = ()

    @property
    def columns(self):
        return self.fields

    @property
    def groups(self):
        return len(self.order) + 1


def family_of(model) -> FMFamily:
    """The trainer's view of a ``DeepFMv2`` (that class itself: a subclass may compute another graph)."""
    from . import models as M
    if type(model) is not M.DeepFMv2:
        raise NotImplementedError("trainer_fm trains DeepFMv2, not %s" % type(model).__name__)
    fields = [(c.key, c.kind, int(c.vocab)) for c in model.id_columns]
    fo = M.first_order_offsets(fields)
    fam = FMFamily(fields, [int(fo[k]) for k, _, _ in fields], list(model.order), int(model.emb_dim), int(model.proj_dim),
                   [int(h) for h in model.hidden], len(model.numeric_keys))
    _check_family(fam)
    return fam


def _check_family(fam: FMFamily):
    keys = [k for k, _, _ in fam.fields]
    if not fam.order or len(set(fam.order)) != len(fam.order) or any(k not in keys for k in fam.order) or len(set(keys)) != len(keys):
        raise ValueError("order must be a non-empty list of distinct field keys")
    G, P = fam.groups, fam.proj_dim
    ok = (1 <= len(fam.fields) <= MAX_FIELDS and 1 <= P <= MAX_PROJ and G * P <= MAX_FLAT and 1 <= len(fam.hidden) <= MAX_LAYERS and
          all(1 <= h <= MAX_WIDTH for h in fam.hidden) and 1 <= fam.emb_dim <= MAX_IN and 0 <= fam.n_dense <= MAX_IN and
          all(v >= 1 for _, _, v in fam.fields))
    if not ok:
        raise ValueError("trainer_fm takes up to %d fields, proj_dim up to %d with groups x proj_dim up to %d, up to %d hidden layers of up to %d units, "
                         "emb_dim and numerics up to %d" % (MAX_FIELDS, MAX_PROJ, MAX_FLAT, MAX_LAYERS, MAX_WIDTH, MAX_IN))
    if lds_bytes(fam, 1) > LDS_BYTES:
        raise ValueError("one sample of this model needs %d bytes of LDS, more than %d" % (lds_bytes(fam, 1), LDS_BYTES))


def param_names(fam: FMFamily):
    """Every trained array -- all of ``DeepFMv2.weight_shapes()`` -- in the order of the device's flat parameter vector: the ``emb/``
    tables in field order and ``fo_cat/kernel`` (the tables), then everything Dense."""
    out = ["emb/" + k for k, _, _ in fam.fields] + ["fo_cat/kernel", "fo_cat/bias", "fo_num/kernel", "fo_num/bias"]
    for k in list(fam.order) + ["num"]:
        out += ["proj/%s/kernel" % k, "proj/%s/bias" % k]
    for i in range(len(fam.hidden)):
        out += ["deep%d/kernel" % i, "deep%d/bias" % i]
    return out + ["head/kernel", "head/bias"]


def param_shapes(fam: FMFamily):
    s = {"emb/" + k: (v, fam.emb_dim) for k, _, v in fam.fields}
    s["fo_cat/kernel"], s["fo_cat/bias"] = (sum(v for _, _, v in fam.fields), 1), (1,)
    s["fo_num/kernel"], s["fo_num/bias"] = (fam.n_dense, 1), (1,)
    for k in fam.order:
        s["proj/%s/kernel" % k], s["proj/%s/bias" % k] = (fam.emb_dim, fam.proj_dim), (fam.proj_dim,)
    s["proj/num/kernel"], s["proj/num/bias"] = (fam.n_dense, fam.proj_dim), (fam.proj_dim,)
    fan = fam.groups * fam.proj_dim
    for i, h in enumerate(fam.hidden):
        s["deep%d/kernel" % i], s["deep%d/bias" % i] = (fan, h), (h,)
        fan = h
    s["head/kernel"], s["head/bias"] = (1 + fam.proj_dim + fam.hidden[-1], 1), (1,)
    return s


def default_tile(fam: FMFamily) -> int:
    """The ``tile`` of a fit that names none (docs/train_fm_results.md has the sweep), halved until the tile fits the LDS."""
    tile = DEFAULT_TILE
    while tile > 1 and lds_bytes(fam, tile) > LDS_BYTES:
        tile //= 2
    return tile


def _wide(fam: FMFamily) -> int:
    return max([fam.groups * fam.proj_dim, 1 + fam.proj_dim + fam.hidden[-1]] + list(fam.hidden))


def lds_bytes(fam: FMFamily, tile: int) -> int:
    """The LDS of one workgroup of the forward + backward kernel, per sample of the tile: the inputs (the groups' table rows and the
    numerics), ``v``, ``s``, ``[first, fm, last activation]``, the other activations, ``d_fm``, ``d_first`` and two gradient buffers."""
    G, P = fam.groups, fam.proj_dim
    per = (G - 1) * fam.emb_dim + fam.n_dense + G * P + P + (1 + P + fam.hidden[-1]) + sum(fam.hidden[:-1]) + P + 1 + 2 * _wide(fam)
    return 4 * int(tile) * per


# ---------------------------------------------------------------- the definition

def _rows(w, key, idc, width):
    """The table rows of a column's ids, zeros for id -1."""
    return np.where((idc >= 0)[:, None], w[key][np.maximum(idc, 0)], _F(0.0)).astype(_F).reshape(len(idc), width)


def forward_host(fam: FMFamily, w, ids, dense, keep: Optional[dict] = None):
    """The definition's probabilities ``[n]`` for packed rows; ``keep`` (a dict) receives every intermediate the backward pass reads."""
    ids, dense = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, col = ids.shape[0], {k: c for c, (k, _, _) in enumerate(fam.fields)}
    with np.errstate(all="ignore"):
        fo_cat = np.zeros((n, 1), dtype=_F)
        for c in sorted(range(len(fam.fields)), key=lambda c: fam.fo_off[c]):
            fo_cat = fo_cat + _rows(w, "fo_cat/kernel", np.where(ids[:, c] >= 0, ids[:, c] + fam.fo_off[c], -1), 1)
        fo_cat = fo_cat + w["fo_cat/bias"][None, :]
        first = fo_cat + _dense(dense, w["fo_num/kernel"], w["fo_num/bias"])
        e = [_rows(w, "emb/" + k, ids[:, col[k]], fam.emb_dim) for k in fam.order] + [dense]
        v = [_dense(e[g], w["proj/%s/kernel" % k], w["proj/%s/bias" % k]) for g, k in enumerate(list(fam.order) + ["num"])]
        s, q = np.zeros((n, fam.proj_dim), dtype=_F), np.zeros((n, fam.proj_dim), dtype=_F)
        for vg in v:
            s = s + vg
            q = q + vg * vg
        fm = s * s - q
        a = np.concatenate(v, axis=1)
        acts = [a]
        for i in range(len(fam.hidden)):
            z = _dense(a, w["deep%d/kernel" % i], w["deep%d/bias" % i])
            a = np.where(z > 0, z, _F(0.0)).astype(_F)
            acts.append(a)
        cat = np.concatenate([first, fm, a], axis=1).astype(_F)
        logit = _dense(cat, w["head/kernel"], w["head/bias"])[:, 0]
        p = sigmoid_def(logit)
    if keep is not None:
        keep.update(e=e, v=v, s=s, fm=fm, first=first, acts=acts, cat=cat, logit=logit)
    return _canonical(p)


def _canonical(a):
    a = np.asarray(a, dtype=_F)
    return np.where(np.isnan(a), QNAN, a).astype(_F)


def step_gradients(fam: FMFamily, w, ids, dense, labels, tile: Optional[int] = None):
    """One step's gradients: ``({name: gradient}, p)`` for the batch ``(ids, dense, labels)`` under the weights ``w``."""
    ids, labels = np.asarray(ids, dtype=np.int32), np.asarray(labels, dtype=_F)
    dense = np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, tile = ids.shape[0], default_tile(fam) if tile is None else int(tile)
    P, L, col = fam.proj_dim, len(fam.hidden), {k: c for c, (k, _, _) in enumerate(fam.fields)}
    k_ = {}
    p = forward_host(fam, w, ids, dense, k_)
    g = {}
    with np.errstate(all="ignore"):
        dz = ((p - labels) / _F(n)).astype(_F)[:, None]
        g["head/kernel"], g["head/bias"] = _grad_kernel(k_["cat"], dz, tile), _grad_bias(dz, tile)
        da = _back(w["head/kernel"], dz)
        d_first, d_fm = da[:, :1], da[:, 1:1 + P]
        dz = np.where(k_["acts"][L] > 0, da[:, 1 + P:], _F(0.0)).astype(_F)
        for i in range(L - 1, -1, -1):
            a = k_["acts"][i]
            g["deep%d/kernel" % i], g["deep%d/bias" % i] = _grad_kernel(a, dz, tile), _grad_bias(dz, tile)
            da = _back(w["deep%d/kernel" % i], dz)
            dz = np.where(a > 0, da, _F(0.0)).astype(_F) if i else da
        for k, _, vocab in fam.fields:
            g["emb/" + k] = np.zeros((vocab, fam.emb_dim), dtype=_F)           # a field outside `order`: no gradient
        for gi, k in enumerate(list(fam.order) + ["num"]):
            vg = k_["v"][gi]
            dv = dz[:, gi * P:(gi + 1) * P] + d_fm * (_F(2.0) * (k_["s"] - vg))
            g["proj/%s/kernel" % k], g["proj/%s/bias" % k] = _grad_kernel(k_["e"][gi], dv, tile), _grad_bias(dv, tile)
            if gi < len(fam.order):
                de = _back(w["proj/%s/kernel" % k], dv)
                g["emb/" + k] = _grad_table(ids[:, col[k]], de, fam.fields[col[k]][2], tile)
        fo = np.zeros((sum(v for _, _, v in fam.fields), 1), dtype=_F)
        for c, (_, _, vocab) in enumerate(fam.fields):
            fo[fam.fo_off[c]:fam.fo_off[c] + vocab] = _grad_table(ids[:, c], d_first, vocab, tile)
        g["fo_cat/kernel"] = fo
        g["fo_cat/bias"] = g["fo_num/bias"] = _grad_bias(d_first, tile)
        g["fo_num/kernel"] = _grad_kernel(dense, d_first, tile)
    return g, p


def adam_step_fm(w, m, v, g, alpha):
    """``trainer.adam_step``, then every NaN of ``w``, ``m`` and ``v`` stored as the quiet NaN."""
    adam_step(w, m, v, g, alpha)
    for a in (w, m, v):
        a[np.isnan(a)] = QNAN


def validate_host(fam: FMFamily, ids, dense, labels):
    """The trainer's checks before the first step, with its messages."""
    _T.validate_host(fam, ids, dense, labels)


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
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else a
    m, v, step = state
    return w, {k: np.array(host(m[k]), dtype=_F) for k in names}, {k: np.array(host(v[k]), dtype=_F) for k in names}, int(step)


def train_host(fam: FMFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
               order=None, tile: Optional[int] = None, state=None) -> TrainResult:
    """The definition on packed host arrays, with ``trainer.train_host``'s arguments and returns: ``ids [N, fields]`` int32 in
    ``model.id_columns`` order, ``dense [N, F]`` float32, ``labels [N]`` float32; ``order`` a permutation of the rows, applied once;
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
    s = L.TrainFmModel()
    s.n_fields, s.n_dense, s.emb_dim, s.proj_dim, s.n_order, s.n_layers = len(fam.fields), fam.n_dense, fam.emb_dim, fam.proj_dim, len(fam.order), len(fam.hidden)
    keys = [k for k, _, _ in fam.fields]
    for c, (_, kind, vocab) in enumerate(fam.fields):
        s.vocab[c], s.genre[c], s.fo_off[c] = vocab, 1 if kind == "genre" else 0, fam.fo_off[c]
    for g, k in enumerate(fam.order):
        s.order[g] = keys.index(k)
    for i, h in enumerate(fam.hidden):
        s.width[i] = h
    return s


def train_device(fam: FMFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
                 order=None, tile: Optional[int] = None, state=None, device=None, workspace=None, num_thresholds: int = 200) -> TrainResult:
    """:func:`train_host` on the device (``sprk_train_fm_fit``): the same bits in every weight, ``m``, ``v`` and ``p``; the history through
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
        need = int(lib.sprk_train_fm_workspace_bytes(C.byref(ms), N, B, tile))
        if workspace is None:
            workspace = torch.empty(max(need, 16) // 8 + 2, dtype=torch.int64, device=dev)
        c1, c2, eps = adam_constants()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if E and N:
            L.check(lib.sprk_train_fm_fit(C.byref(ms), ptr(ids), ptr(dense) if fam.n_dense else None, ptr(labels), ptr(order_t) if order is not None else None,
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
