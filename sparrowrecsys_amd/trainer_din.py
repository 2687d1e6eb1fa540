"""``trainer_din.fit(model, ...)`` for ``DIN`` -- an attention unit shared over the T history slots, PReLU with trained ``alpha``, a weighted
sum pooling, one movie table read through T + 1 id columns -- trained with Adam under the rules of :mod:`trainer` (DESIGN.md sections
5.12 and 5.19).

:func:`train_host` is the DEFINITION, in numpy with a fixed operation order; ``sprk_train_din_fit`` (csrc/k_train_din.h,
csrc/api_train_din.h) computes the same bits on the device.  The arithmetic is the trainer's own, through the trainer's own functions:
float32, every product and sum rounded on its own, no fused multiply-add, sums from ``+0`` in index order, ``sigmoid_def``, the two-level
gradient sums (a tile's samples, then the tiles), Adam over every element on every step, ``alpha_t`` in doubles on the host, ``order``
applied once; non-finite inputs and ids outside the vocabulary are errors found before the first step.  What this graph adds
(``T = hist_len``, ``D = emb_dim``, ``H = att_hidden``; ``ids [N, T + 4]`` in ``model.id_columns`` order: ``movieId``,
``userRatedMovie1..T``, ``userId``, ``userGenre1``, ``movieGenre1``; ``dense [N, 7]`` in ``model.numeric_keys`` order):

Forward.

* ``c = movie[movieId]``, ``h_t = movie[hist_t]``: history id 0 gathers row 0 and trains it -- no masking, as ``models.DIN`` and
  ``oracle.ctr_oracle.din_forward`` read the reference; a genre id of -1 gives a zero row;
* ``a_t = [h_t - c | h_t | c | h_t c]`` (DIN.py:146), ``u_t = _dense(a_t, att0)``, ``y_t = PReLU(u_t, alpha[t])``,
  ``s_t = sigmoid_def(_dense(y_t, att1))``;
* ``pooled = ((+0 + h_0 s_0) + h_1 s_1) + ...`` in slot order;
* the tail's input is laid out by ``DIN._fc_rows()``; ``PReLU(_dense(., fc{i}), fc{i}_prelu/alpha)`` per layer; ``p = sigmoid_def(_dense(., head))``;
* PReLU is ``z`` where ``z > 0``, ``alpha z`` where ``z < 0``, else ``+0``.

Backward.

* ``dlogit = (p - y) / n`` as in :mod:`trainer`; a Dense layer's input gradient is ``_back``;
* PReLU as TensorFlow differentiates ``relu(x) - alpha relu(-x)``: ``dz = dy`` where ``z > 0``, ``alpha dy`` where ``z < 0``, ``+0`` at
  ``z == 0``; ``dalpha`` gets ``dy z`` where ``z < 0``, else ``+0``;
* the attention sigmoid: ``ds_t = sum_d dpooled_d h_td`` in ``d`` order from ``+0``; its logit's gradient is ``(ds_t s_t) (1 - s_t)``;
  with ``dA_t = _back(att0/kernel, du_t)`` in the four blocks ``[h - c | h | c | h c]``;
* the gradient that reaches a gathered row is one fixed expression per element: history slot ``t``:
  ``((dpooled_d s_t + dA_t[h - c]_d) + dA_t[h]_d) + dA_t[h c]_d c_d``; the candidate: ``x = `` the ``fc0`` input row's gradient, then for
  ``t = 0 .. T - 1`` in order ``x = ((x - dA_t[h - c]_d) + dA_t[c]_d) + dA_t[h c]_d h_td``; any other column: its ``fc0`` input rows' gradient.

Sums over samples.

* a parameter that is no table is summed over a tile's samples from ``+0``: ``att0/*`` and ``att1/*`` over the tile's ``(sample, slot)``
  pairs, sample-major; ``att_prelu/alpha[t]`` over the tile's samples; then the tiles are added from ``+0``;
* a table row is summed over the entries ``(sample, column)`` of the batch that carry its id in a column of that table: within a tile
  in ``(sample, column)`` order from ``+0``, then the tiles from ``+0``.  A sample whose candidate also sits in two history slots
  contributes three entries to one row in one tile.

No stored value is changed on its way out: a NaN keeps the bits the arithmetic gave it (nothing here is canonicalised; finite inputs and
weights of ordinary size produce none).
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np

from . import trainer as _T
from .trainer import (DEFAULT_BATCH, LDS_BYTES, TrainResult, _back, _check_args, _check_order, _dense, _error_message, _grad_bias, _grad_kernel, _grad_table,
                      adam_alpha, adam_constants, adam_step, sigmoid_def)

MAX_COLS, MAX_TABLES, MAX_LAYERS, MAX_X, MAX_WIDTH, MAX_EMB = 16, 16, 8, 256, 256, 64
MAX_HIST = MAX_COLS - 4
MAX_BATCH = 1 << 28                                                   # the schedule's keys hold position x 16 + column in 32 bits
DEFAULT_TILE = 4                                                      # chosen from the tile sweep in docs/train_din_results.md
SRC_NUMERIC, SRC_POOLED = -1, -2
_F = np.float32


class DinFamily(namedtuple("DinFamily", "columns tables table_of emb_dim hist_len att_hidden hidden n_dense xsrc xsub")):
    """``columns``: ``(key, kind, vocab)`` in ``model.id_columns`` order (the candidate, the T history slots, then the others);
    ``tables``: the trained tables' names; ``table_of``: per column the index of the table it reads; per ``fc0`` input row its source
    ``xsrc`` (an id column, ``SRC_NUMERIC`` or ``SRC_POOLED``) and ``xsub`` (the element of the row, of the numerics, of the pooled vector)."""
    __slots__ = ()

    @property
    def fan0(self):
        return len(self.xsrc)


def family_of(model) -> DinFamily:
    """The trainer's view of a ``DIN`` (that class itself: DIEN and any other subclass compute another graph)."""
    from . import models as M
    if type(model) is not M.DIN:
        raise NotImplementedError("trainer_din trains DIN, not %s" % type(model).__name__)
    T, D = int(model.hist_len), int(model.emb_dim)
    cols = [(c.key, c.kind, int(c.vocab)) for c in model.id_columns]
    keys = [k for k, _, _ in cols]
    rows, fan = model._fc_rows()
    xsrc, xsub = [None] * fan, [None] * fan
    for name, (r0, width) in rows.items():
        if name == "__pooled__":
            src = SRC_POOLED
        elif name == "__cand__":
            src = 0
        elif name.endswith("_embedding"):
            src = keys.index(name[:-len("_embedding")])
        else:
            src = SRC_NUMERIC
        for j in range(width):
            xsrc[r0 + j], xsub[r0 + j] = src, (list(model.numeric_keys).index(name) if src == SRC_NUMERIC else j)
    fam = DinFamily(cols, ["emb/movie", "emb/userId", "emb/userGenre1", "emb/movieGenre1"], [0] * (T + 1) + [1, 2, 3], D, T, int(model.att_hidden),
                    [int(h) for h in model.hidden], len(model.numeric_keys), xsrc, xsub)
    _check_family(fam)
    return fam


def _check_family(fam: DinFamily):
    T, C = fam.hist_len, len(fam.columns)
    ok = (1 <= T <= MAX_HIST and T + 1 <= C <= MAX_COLS and len(fam.table_of) == C and 1 <= len(fam.tables) <= MAX_TABLES and
          1 <= fam.emb_dim <= MAX_EMB and 1 <= fam.att_hidden <= MAX_WIDTH and 1 <= len(fam.hidden) <= MAX_LAYERS and
          all(1 <= h <= MAX_WIDTH for h in fam.hidden) and 1 <= fam.fan0 <= MAX_X and 0 <= fam.n_dense <= MAX_X and all(v >= 1 for _, _, v in fam.columns))
    if not ok:
        raise ValueError("trainer_din takes up to %d id columns (hist_len up to %d), emb_dim up to %d, att_hidden up to %d, up to %d tail layers of up to %d units "
                         "and %d fc0 input rows" % (MAX_COLS, MAX_HIST, MAX_EMB, MAX_WIDTH, MAX_LAYERS, MAX_WIDTH, MAX_X))
    if any(fam.table_of[c] != 0 for c in range(T + 1)) or sorted(set(fam.table_of)) != list(range(len(fam.tables))):
        raise ValueError("the candidate and the history slots read table 0, and every table is read by a column")
    for c, (_, kind, vocab) in enumerate(fam.columns):
        first = fam.table_of.index(fam.table_of[c])
        if fam.columns[first][1:] != (kind, vocab):
            raise ValueError("the columns of one table share its vocabulary and kind")
    for src in [SRC_POOLED, 0] + list(range(T + 1, C)):
        if sorted(sub for s, sub in zip(fam.xsrc, fam.xsub) if s == src) != list(range(fam.emb_dim)):
            raise ValueError("fc0's input holds the pooled vector, the candidate and every column behind the history once each")
    if any(s != SRC_NUMERIC and s != SRC_POOLED and not (s == 0 or T < s < C) for s in fam.xsrc) or any(
            s == SRC_NUMERIC and not 0 <= sub < fam.n_dense for s, sub in zip(fam.xsrc, fam.xsub)):
        raise ValueError("an fc0 input row names a history column, or a numeric outside the numerics")
    if lds_bytes(fam, 1) > LDS_BYTES:
        raise ValueError("one sample of this model needs %d bytes of LDS, more than %d" % (lds_bytes(fam, 1), LDS_BYTES))


def _table_vocab(fam: DinFamily, t: int) -> int:
    return fam.columns[fam.table_of.index(t)][2]


def param_names(fam: DinFamily):
    """Every trained array -- all of ``DIN.weight_shapes()`` -- in the order of the device's flat parameter vector: the tables, the
    attention unit, the tail, the head."""
    out = list(fam.tables) + ["att0/kernel", "att0/bias", "att_prelu/alpha", "att1/kernel", "att1/bias"]
    for i in range(len(fam.hidden)):
        out += ["fc%d/kernel" % i, "fc%d/bias" % i, "fc%d_prelu/alpha" % i]
    return out + ["head/kernel", "head/bias"]


def param_shapes(fam: DinFamily):
    D, T, H = fam.emb_dim, fam.hist_len, fam.att_hidden
    s = {name: (_table_vocab(fam, t), D) for t, name in enumerate(fam.tables)}
    s.update({"att0/kernel": (4 * D, H), "att0/bias": (H,), "att_prelu/alpha": (T, H), "att1/kernel": (H, 1), "att1/bias": (1,)})
    fan = fam.fan0
    for i, h in enumerate(fam.hidden):
        s["fc%d/kernel" % i], s["fc%d/bias" % i], s["fc%d_prelu/alpha" % i] = (fan, h), (h,), (h,)
        fan = h
    s["head/kernel"], s["head/bias"] = (fan, 1), (1,)
    return s


def default_tile(fam: DinFamily) -> int:
    """The ``tile`` of a fit that names none (docs/train_din_results.md has the sweep), halved until the tile fits the LDS."""
    tile = DEFAULT_TILE
    while tile > 1 and lds_bytes(fam, tile) > LDS_BYTES:
        tile //= 2
    return tile


def _wide(fam: DinFamily) -> int:
    return max(list(fam.hidden) + [fam.hist_len * fam.att_hidden, 4 * fam.hist_len * fam.emb_dim])


def lds_bytes(fam: DinFamily, tile: int) -> int:
    """The LDS of one workgroup of the forward + backward kernel, per sample of the tile: the T + 1 gathered movie rows, the attention
    pre-activations ``[T][H]``, ``s`` and its logit's gradient ``[T]`` each, the ``fc0`` input and its gradient, every tail layer's
    pre-activation and activation, and two gradient buffers as wide as the widest of a tail layer, ``T H`` and ``4 T D``; then, once per
    workgroup, ``att0/kernel``, ``att0/bias``, ``att_prelu/alpha`` and ``att1/kernel``."""
    T, D, H = fam.hist_len, fam.emb_dim, fam.att_hidden
    per = (T + 1) * D + T * H + 2 * T + 2 * fam.fan0 + 2 * sum(fam.hidden) + 2 * _wide(fam)
    return 4 * (int(tile) * per + 4 * D * H + H + T * H + H)


# ---------------------------------------------------------------- the definition

def prelu(z, alpha):
    """``z`` where ``z > 0``, ``alpha z`` where ``z < 0``, else ``+0``."""
    with np.errstate(all="ignore"):
        return np.where(z > 0, z, np.where(z < 0, alpha * z, _F(0.0))).astype(_F)


def prelu_back(z, alpha, dy):
    """-> ``(dz, dalpha's terms)``: ``dy`` / ``alpha dy`` / ``+0`` and ``+0`` / ``dy z`` / ``+0`` where ``z`` is positive / negative / neither."""
    with np.errstate(all="ignore"):
        dz = np.where(z > 0, dy, np.where(z < 0, alpha * dy, _F(0.0))).astype(_F)
        da = np.where(z < 0, dy * z, _F(0.0)).astype(_F)
    return dz, da


def _rows(table, idc):
    """The table rows of a column's ids, zeros for id -1."""
    return np.where((idc >= 0)[:, None], table[np.maximum(idc, 0)], _F(0.0)).astype(_F)


def forward_host(fam: DinFamily, w, ids, dense, keep: Optional[dict] = None):
    """The definition's probabilities ``[n]`` for packed rows; ``keep`` (a dict) receives every intermediate the backward pass reads."""
    ids, dense = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, T, D, H = ids.shape[0], fam.hist_len, fam.emb_dim, fam.att_hidden
    with np.errstate(all="ignore"):
        rows = [_rows(w[fam.tables[fam.table_of[c]]], ids[:, c]) for c in range(len(fam.columns))]
        c = rows[0]
        h = np.stack(rows[1:T + 1], axis=1).reshape(n, T, D)
        cr = np.broadcast_to(c[:, None, :], (n, T, D))
        a = np.concatenate([h - cr, h, cr, h * cr], axis=2).astype(_F)
        u = _dense(a.reshape(n * T, 4 * D), w["att0/kernel"], w["att0/bias"]).reshape(n, T, H)
        ya = prelu(u, w["att_prelu/alpha"][None])
        s = sigmoid_def(_dense(ya.reshape(n * T, H), w["att1/kernel"], w["att1/bias"])[:, 0]).reshape(n, T)
        pooled = np.zeros((n, D), dtype=_F)
        for t in range(T):
            pooled = pooled + h[:, t] * s[:, t, None]
        x = np.zeros((n, fam.fan0), dtype=_F)
        for k, (src, sub) in enumerate(zip(fam.xsrc, fam.xsub)):
            x[:, k] = dense[:, sub] if src == SRC_NUMERIC else pooled[:, sub] if src == SRC_POOLED else rows[src][:, sub]
        acts, zs = [x], []
        for i in range(len(fam.hidden)):
            z = _dense(acts[-1], w["fc%d/kernel" % i], w["fc%d/bias" % i])
            zs.append(z)
            acts.append(prelu(z, w["fc%d_prelu/alpha" % i][None]))
        logit = _dense(acts[-1], w["head/kernel"], w["head/bias"])[:, 0]
        p = sigmoid_def(logit)
    if keep is not None:
        keep.update(c=c, h=h, a=a, u=u, ya=ya, s=s, pooled=pooled, acts=acts, zs=zs, logit=logit)
    return p


def _grad_rows(idc, dxc, vocab, tile):
    """``trainer._grad_table`` over the entries ``(sample, column)`` of the columns that read one table: ``idc [n, k]``, ``dxc [n, k, D]``.
    The entries in sample-major order are a column of ``n k`` ids in tiles of ``tile k``."""
    n, k = idc.shape
    return _grad_table(idc.reshape(n * k), dxc.reshape(n * k, dxc.shape[2]), vocab, tile * k)


def step_gradients(fam: DinFamily, w, ids, dense, labels, tile: Optional[int] = None, keep: Optional[dict] = None):
    """One step's gradients: ``({name: gradient}, p)`` for the batch ``(ids, dense, labels)`` under the weights ``w``; ``keep`` receives
    the forward's intermediates and the per-``(sample, column)`` row gradients ``drow [n, C, D]``."""
    ids, labels = np.asarray(ids, dtype=np.int32), np.asarray(labels, dtype=_F)
    dense = np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, tile = ids.shape[0], default_tile(fam) if tile is None else int(tile)
    T, D, H, L, C = fam.hist_len, fam.emb_dim, fam.att_hidden, len(fam.hidden), len(fam.columns)
    k_ = {}
    p = forward_host(fam, w, ids, dense, k_)
    g = {}
    with np.errstate(all="ignore"):
        dz = ((p - labels) / _F(n)).astype(_F)[:, None]
        g["head/kernel"], g["head/bias"] = _grad_kernel(k_["acts"][L], dz, tile), _grad_bias(dz, tile)
        dy = _back(w["head/kernel"], dz)
        for i in range(L - 1, -1, -1):
            dz, dal = prelu_back(k_["zs"][i], w["fc%d_prelu/alpha" % i][None], dy)
            g["fc%d_prelu/alpha" % i] = _grad_bias(dal, tile)
            g["fc%d/kernel" % i], g["fc%d/bias" % i] = _grad_kernel(k_["acts"][i], dz, tile), _grad_bias(dz, tile)
            dy = _back(w["fc%d/kernel" % i], dz)
        dx = dy                                                                  # [n, fan0]
        col_rows = lambda src: [k for _, k in sorted((fam.xsub[k], k) for k in range(fam.fan0) if fam.xsrc[k] == src)]
        pr = col_rows(SRC_POOLED)
        dpooled = dx[:, pr] if len(pr) == D else np.zeros((n, D), dtype=_F)
        h, c, s = k_["h"], k_["c"], k_["s"]
        ds = np.zeros((n, T), dtype=_F)
        for d in range(D):
            ds = ds + dpooled[:, d, None] * h[:, :, d]
        dl = ((ds * s) * (_F(1.0) - s)).astype(_F).reshape(n * T, 1)
        ya, u, a = k_["ya"].reshape(n * T, H), k_["u"], k_["a"].reshape(n * T, 4 * D)
        g["att1/kernel"], g["att1/bias"] = _grad_kernel(ya, dl, tile * T), _grad_bias(dl, tile * T)
        dya = _back(w["att1/kernel"], dl).reshape(n, T, H)
        du, dal = prelu_back(u, w["att_prelu/alpha"][None], dya)
        g["att_prelu/alpha"] = _grad_bias(dal.reshape(n, T * H), tile).reshape(T, H)
        du = du.reshape(n * T, H)
        g["att0/kernel"], g["att0/bias"] = _grad_kernel(a, du, tile * T), _grad_bias(du, tile * T)
        dA = _back(w["att0/kernel"], du).reshape(n, T, 4, D)
        drow = np.zeros((n, C, D), dtype=_F)
        for cc in range(C):
            ks = col_rows(cc)
            if len(ks) == D:
                drow[:, cc] = dx[:, ks]
        x = drow[:, 0].copy()
        for t in range(T):
            drow[:, 1 + t] = ((dpooled * s[:, t, None] + dA[:, t, 0]) + dA[:, t, 1]) + dA[:, t, 3] * c
            x = ((x - dA[:, t, 0]) + dA[:, t, 2]) + dA[:, t, 3] * h[:, t]
        drow[:, 0] = x
        for t, name in enumerate(fam.tables):
            cs = [cc for cc in range(C) if fam.table_of[cc] == t]
            g[name] = _grad_rows(ids[:, cs], drow[:, cs], _table_vocab(fam, t), tile)
    if keep is not None:
        keep.update(k_, dx=dx, dA=dA, drow=drow, dpooled=dpooled, ds=ds, dl=dl.reshape(n, T))
    return g, p


def validate_host(fam: DinFamily, ids, dense, labels):
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


def train_host(fam: DinFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
               order=None, tile: Optional[int] = None, state=None) -> TrainResult:
    """The definition on packed host arrays, with ``trainer.train_host``'s arguments and returns: ``ids [N, T + 4]`` int32 in
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
    if B > MAX_BATCH:
        raise ValueError("batch_size = %d: the schedule's keys take batches of up to 2^28 rows" % B)
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
    s = L.TrainDinModel()
    s.n_cols, s.n_dense, s.emb_dim, s.hist_len, s.att_hidden, s.n_x, s.n_layers = (len(fam.columns), fam.n_dense, fam.emb_dim, fam.hist_len, fam.att_hidden,
                                                                                  fam.fan0, len(fam.hidden))
    for c, (_, kind, vocab) in enumerate(fam.columns):
        s.vocab[c], s.genre[c], s.table[c] = vocab, 1 if kind == "genre" else 0, fam.table_of[c]
    for i, h in enumerate(fam.hidden):
        s.width[i] = h
    for k, (src, sub) in enumerate(zip(fam.xsrc, fam.xsub)):
        s.xsrc[k], s.xsub[k] = src, sub
    return s


def train_device(fam: DinFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
                 order=None, tile: Optional[int] = None, state=None, device=None, workspace=None, num_thresholds: int = 200) -> TrainResult:
    """:func:`train_host` on the device (``sprk_train_din_fit``): the same bits in every weight, ``m``, ``v`` and ``p``; the history through
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
        if B > MAX_BATCH:
            raise ValueError("batch_size = %d: the schedule's keys take batches of up to 2^28 rows" % B)
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
        need = int(lib.sprk_train_din_workspace_bytes(C.byref(ms), N, B, tile))
        if workspace is None:
            workspace = torch.empty(max(need, 16) // 8 + 2, dtype=torch.int64, device=dev)
        c1, c2, eps = adam_constants()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if E and N:
            L.check(lib.sprk_train_din_fit(C.byref(ms), ptr(ids), ptr(dense) if fam.n_dense else None, ptr(labels), ptr(order_t) if order is not None else None,
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
    """``CTRModel.fit`` for a ``DIN``: the same arguments (a dict of columns with ``"label"`` or ``y``, or an iterable of ``(features,
    labels)`` batches) and the same return value (per epoch ``[loss, accuracy, roc_auc, pr_auc]``); the trained weights are set on
    ``model`` and Adam's moments kept in ``model._fit_state``, so a second call continues.  This function is the entry: ``DIN.fit``
    itself still raises ``NotImplementedError`` (DESIGN.md section 5.19 says what its one-line dispatch waits on)."""
    import sys
    fam = family_of(model)
    return model._fit_with(sys.modules[__name__], fam, x, y, batch_size, epochs, learning_rate, order, tile)
