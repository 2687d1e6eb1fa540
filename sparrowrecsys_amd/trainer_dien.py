"""``trainer_dien.fit(model, ...)`` for ``DIEN`` -- a Keras GRU over the T history slots that consumes the embedding's zero mask, a sigmoid
attention gate per slot, the reference's hand-written AUGRU, a PReLU tail -- trained with Adam under the rules of :mod:`trainer` and in the
shape of :mod:`trainer_din` (DESIGN.md sections 5.12, 5.19 and 5.22).

:func:`train_host` is the DEFINITION, in numpy with a fixed operation order; ``sprk_train_dien_fit`` (csrc/k_train_dien.h,
csrc/api_train_dien.h) computes the same bits on the device.  The arithmetic is the trainer's own, through the trainer's own functions:
float32, every product and sum rounded on its own, no fused multiply-add, sums from ``+0`` in index order, ``sigmoid_def``, the two-level
gradient sums (a tile's samples, then the tiles), Adam over every element on every step, ``alpha_t`` in doubles on the host, ``order``
applied once; non-finite inputs and ids outside the vocabulary are errors found before the first step.  What this graph adds
(``T = hist_len``, ``D = emb_dim``, ``H = att_hidden``; ``ids [N, T + 4]`` in ``model.id_columns`` order: ``movieId``,
``userRatedMovie1..T``, ``userId``, ``userGenre1``, ``movieGenre1``; ``dense [N, 7]`` in ``model.numeric_keys`` order):

Forward (``oracle.ctr_oracle.dien_forward``'s graph).

* ``tanh_def(z) = (s + s) - 1`` with ``s = sigmoid_def(z + z)``: no libm; ``z + z`` and ``s + s`` are exact, ``tanh_def(0) = 0`` exactly;
* ``c = movie[movieId]``, ``x_t = movie[hist_t]``; slot ``t`` is masked where ``hist_t == 0``;
* the GRU (Keras, ``reset_after=True``, gates ``z | r | h``, bias rows input / recurrent): ``mx = _dense(x_t, gru/kernel, gru/bias[0])``,
  ``mh = _dense(h, gru_rec/kernel, gru/bias[1])``, ``z = sigmoid_def(mx_z + mh_z)``, ``r = sigmoid_def(mx_r + mh_r)``,
  ``hh = tanh_def(mx_h + r mh_h)``, ``hn = z h + (1 - z) hh``; the state ``h`` starts at ``+0``.  At an unmasked slot ``h = hn`` and the
  output ``g_t = hn``; at a masked slot the state is kept and ``g_t = g_{t-1}`` (``+0`` before the first unmasked slot);
* the attention gate: ``q_t = g_t c``, ``y_t = sigmoid_def(_dense(q_t, att0))``, ``a_t = sigmoid_def(_dense(y_t, att1))``, one scalar per slot;
* the AUGRU, as the reference writes it: per gate ``pre = _dense(g_t, in) + hid @ hid_kernel`` (the second product in ``_dense``'s ``k``
  order from ``+0``, no bias), ``r_t = sigmoid_def(_dense(pre_r, out_r))`` and ``z_t`` likewise with ``hid = hs``;
  ``hc_t = tanh_def(_dense(pre_h, out_h))`` with ``hid = hs z_t``; ``u_t = a_t r_t``; ``hs <- (1 - u_t) hs + u_t hc_t``; ``hs`` starts as
  ``augru/h0`` for every sample;
* the tail's input is laid out by ``DIEN._fc_rows()`` (the last ``hs`` where DIN has the pooled vector); the tail, PReLU and the head are
  :mod:`trainer_din`'s.

Backward.  ``dlogit``, the head, the tail and PReLU as in :mod:`trainer_din`; ``dx`` is ``fc0``'s input gradient.  A sigmoid ``s`` with
output gradient ``ds`` has the logit gradient ``(ds s) (1 - s)``; a ``tanh_def`` output ``y`` with gradient ``dy`` has ``dy (1 - y y)``.
Every gradient with more than one source is one fixed expression per element, the additions in the order written:

* the AUGRU walks ``t = T - 1 .. 0`` with ``dhs`` (``fc0``'s input rows of the last ``hs`` to begin with); ``hs`` is the state BEFORE slot ``t``:
  ``du = dhs (hc_t - hs)``, ``dhc = dhs u_t``, ``da_t = sum_d du_d r_td`` in ``d`` order from ``+0``, ``dr = du a_t``;
  ``do_h = dhc (1 - hc_t hc_t)``, ``dpre_h = _back(out_h/kernel, do_h)``, ``dhz = _back(hid_h/kernel, dpre_h)``, ``dz = dhz hs``;
  ``do_z = (dz z_t) (1 - z_t)``, ``do_r = (dr r_t) (1 - r_t)``, ``dpre_g = _back(out_g/kernel, do_g)``;
  ``hs`` receives ``((dhs (1 - u_t) + _back(hid_r/kernel, dpre_r)) + _back(hid_z/kernel, dpre_z)) + dhz z_t``, the next ``dhs``;
  what is left after slot 0 is ``augru/h0``'s per-sample term;
* the gate: ``dl_t = (da_t a_t) (1 - a_t)``, ``dy_t = _back(att1/kernel, dl_t)``, ``de_t = (dy_t y_t) (1 - y_t)``, ``dq_t = _back(att0/kernel, de_t)``;
* ``g_t`` receives ``dg_t = ((dq_t c + _back(in_r/kernel, dpre_r)) + _back(in_z/kernel, dpre_z)) + _back(in_h/kernel, dpre_h)``;
* the candidate's row receives ``x = `` its ``fc0`` input rows' gradient, then for ``t = 0 .. T - 1`` in order ``x = x + dq_t g_t``;
* the masked GRU walks ``t = T - 1 .. 0`` with a state gradient ``dh`` and a held-output gradient ``do``, both from ``+0``: at every slot
  ``do = do + dg_t``; at an unmasked slot ``dhn = dh + do`` and ``do`` returns to ``+0``, ``dzg = dhn (h - hh)``, ``dhh = dhn (1 - z)``,
  ``dp_h = dhh (1 - hh hh)``, ``dr = dp_h mh_h``, ``dp_z = (dzg z) (1 - z)``, ``dp_r = (dr r) (1 - r)``, ``dmx = [dp_z | dp_r | dp_h]``,
  ``dmh = [dp_z | dp_r | dp_h r]``, the slot's row receives ``_back(gru/kernel, dmx)`` and the state ``dh = dhn z + _back(gru_rec/kernel, dmh)``
  (``h`` the state before the slot); at a masked slot ``dh`` passes unchanged, ``dmx = dmh = +0`` and the slot's row receives ``+0`` in every
  element; what is left in ``do`` below the first unmasked slot is dropped;
* any other column: its ``fc0`` input rows' gradient.

Sums over samples.

* a parameter used once per ``(sample, slot)`` -- the GRU arrays, ``att0/*``, ``att1/*``, all AUGRU arrays -- is summed over the tile's
  pairs sample-major from ``+0`` (``_grad_kernel`` / ``_grad_bias`` over ``[n T]`` rows in tiles of ``tile T``), then the tiles from ``+0``;
  a masked GRU slot's terms are products with ``+0``;
* ``augru/h0`` over the tile's samples, then the tiles; the tail and the head as in :mod:`trainer_din`;
* a table row over the entries ``(sample, column)`` of the batch that carry its id in a column of that table: within a tile in
  ``(sample, column)`` order from ``+0``, then the tiles from ``+0``.  A masked slot is an entry of row 0 that carries ``+0``: a sum from
  ``+0`` is unchanged by it, so row 0 of ``emb/movie`` moves only through the candidate column (and the device's schedule leaves such
  entries out: the same bits).

The loss is the binary cross-entropy of ``y_pred``; the reference's auxiliary loss is left out and ``augru/h0`` is trained (DESIGN.md
section 5.22).  No stored value is changed on its way out (nothing here is canonicalised).
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np

from . import trainer as _T
from .trainer import (DEFAULT_BATCH, LDS_BYTES, TrainResult, _back, _check_args, _check_order, _dense, _error_message, _grad_bias, _grad_kernel,
                      adam_alpha, adam_constants, adam_step, sigmoid_def)
from .trainer_din import (MAX_BATCH, MAX_COLS, MAX_EMB, MAX_HIST, MAX_LAYERS, MAX_TABLES, MAX_WIDTH, MAX_X, SRC_NUMERIC, SRC_POOLED, _grad_rows, _rows, prelu,
                          prelu_back)

DEFAULT_TILE = 8                                                      # chosen from the tile sweep 1, 2, 4, 8, 16 in docs/train_dien_results.md
STAGE_EMB = 16                                                        # the recurrent weights are staged in LDS up to this emb_dim (15 D D + 12 D floats)
GATES = ("r", "z", "h")
_F = np.float32


class DienFamily(namedtuple("DienFamily", "columns tables table_of emb_dim hist_len att_hidden hidden n_dense xsrc xsub")):
    """``trainer_din.DinFamily``'s fields; ``SRC_POOLED`` names the AUGRU's last state."""
    __slots__ = ()

    @property
    def fan0(self):
        return len(self.xsrc)


def family_of(model) -> DienFamily:
    """The trainer's view of a ``DIEN`` (that class itself)."""
    from . import models as M
    if type(model) is not M.DIEN:
        raise NotImplementedError("trainer_dien trains DIEN, not %s" % type(model).__name__)
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
    fam = DienFamily(cols, ["emb/movie", "emb/userId", "emb/userGenre1", "emb/movieGenre1"], [0] * (T + 1) + [1, 2, 3], D, T, int(model.att_hidden),
                     [int(h) for h in model.hidden], len(model.numeric_keys), xsrc, xsub)
    _check_family(fam)
    return fam


def _check_family(fam: DienFamily):
    T, C = fam.hist_len, len(fam.columns)
    ok = (1 <= T <= MAX_HIST and T + 1 <= C <= MAX_COLS and len(fam.table_of) == C and 1 <= len(fam.tables) <= MAX_TABLES and
          1 <= fam.emb_dim <= MAX_EMB and 1 <= fam.att_hidden <= MAX_WIDTH and 1 <= len(fam.hidden) <= MAX_LAYERS and
          all(1 <= h <= MAX_WIDTH for h in fam.hidden) and 1 <= fam.fan0 <= MAX_X and 0 <= fam.n_dense <= MAX_X and all(v >= 1 for _, _, v in fam.columns))
    if not ok:
        raise ValueError("trainer_dien takes up to %d id columns (hist_len up to %d), emb_dim up to %d, att_hidden up to %d, up to %d tail layers of up to %d units "
                         "and %d fc0 input rows" % (MAX_COLS, MAX_HIST, MAX_EMB, MAX_WIDTH, MAX_LAYERS, MAX_WIDTH, MAX_X))
    if any(fam.table_of[c] != 0 for c in range(T + 1)) or sorted(set(fam.table_of)) != list(range(len(fam.tables))):
        raise ValueError("the candidate and the history slots read table 0, and every table is read by a column")
    if fam.columns[0][1] != "id":
        raise ValueError("the movie columns hold ids from 0, of which 0 masks a history slot")
    for c, (_, kind, vocab) in enumerate(fam.columns):
        first = fam.table_of.index(fam.table_of[c])
        if fam.columns[first][1:] != (kind, vocab):
            raise ValueError("the columns of one table share its vocabulary and kind")
    for src in [SRC_POOLED, 0] + list(range(T + 1, C)):
        if sorted(sub for s, sub in zip(fam.xsrc, fam.xsub) if s == src) != list(range(fam.emb_dim)):
            raise ValueError("fc0's input holds the AUGRU's state, the candidate and every column behind the history once each")
    if any(s != SRC_NUMERIC and s != SRC_POOLED and not (s == 0 or T < s < C) for s in fam.xsrc) or any(
            s == SRC_NUMERIC and not 0 <= sub < fam.n_dense for s, sub in zip(fam.xsrc, fam.xsub)):
        raise ValueError("an fc0 input row names a history column, or a numeric outside the numerics")
    if lds_bytes(fam, 1) > LDS_BYTES:
        raise ValueError("one sample of this model needs %d bytes of LDS, more than %d" % (lds_bytes(fam, 1), LDS_BYTES))


def _table_vocab(fam: DienFamily, t: int) -> int:
    return fam.columns[fam.table_of.index(t)][2]


def param_names(fam: DienFamily):
    """Every trained array -- all of ``DIEN.weight_shapes()`` -- in the order of the device's flat parameter vector: the tables, the GRU,
    the attention gate, the AUGRU's three gates and its initial state, the tail, the head."""
    out = list(fam.tables) + ["gru/kernel", "gru_rec/kernel", "gru/bias", "att0/kernel", "att0/bias", "att1/kernel", "att1/bias"]
    for g in GATES:
        out += ["augru_%s_in/kernel" % g, "augru_%s_in/bias" % g, "augru_%s_hid/kernel" % g, "augru_%s_out/kernel" % g, "augru_%s_out/bias" % g]
    out.append("augru/h0")
    for i in range(len(fam.hidden)):
        out += ["fc%d/kernel" % i, "fc%d/bias" % i, "fc%d_prelu/alpha" % i]
    return out + ["head/kernel", "head/bias"]


def param_shapes(fam: DienFamily):
    D, H = fam.emb_dim, fam.att_hidden
    s = {name: (_table_vocab(fam, t), D) for t, name in enumerate(fam.tables)}
    s.update({"gru/kernel": (D, 3 * D), "gru_rec/kernel": (D, 3 * D), "gru/bias": (2, 3 * D),
              "att0/kernel": (D, H), "att0/bias": (H,), "att1/kernel": (H, 1), "att1/bias": (1,)})
    for g in GATES:
        s.update({"augru_%s_in/kernel" % g: (D, D), "augru_%s_in/bias" % g: (D,), "augru_%s_hid/kernel" % g: (D, D), "augru_%s_out/kernel" % g: (D, D),
                  "augru_%s_out/bias" % g: (D,)})
    s["augru/h0"] = (1, D)
    fan = fam.fan0
    for i, h in enumerate(fam.hidden):
        s["fc%d/kernel" % i], s["fc%d/bias" % i], s["fc%d_prelu/alpha" % i] = (fan, h), (h,), (h,)
        fan = h
    s["head/kernel"], s["head/bias"] = (fan, 1), (1,)
    return s


def default_tile(fam: DienFamily) -> int:
    """The ``tile`` of a fit that names none, halved until the tile fits the LDS."""
    tile = DEFAULT_TILE
    while tile > 1 and lds_bytes(fam, tile) > LDS_BYTES:
        tile //= 2
    return tile


def lds_bytes(fam: DienFamily, tile: int) -> int:
    """The LDS of one workgroup of the forward + backward kernel.  Per sample of the tile, in floats: the T + 1 gathered movie rows; per
    slot the GRU's state before the slot, ``z``, ``r``, ``hh``, ``mh_h`` and the output ``g`` (``6 T D``); the gate's ``y [T][H]`` and
    ``a [T]``; per slot the AUGRU's state before the slot, ``r_t``, ``z_t``, ``hc_t`` and the three ``pre`` (``7 T D``); the backward walk's
    ``do`` and ``dpre`` of the three gates (``6 T D``, used again for the GRU's ``dmx`` and ``dmh``), ``dq`` and ``dg`` (``2 T D``),
    ``dl [T]`` and ``de [T][H]``; eight vectors of ``D`` for the walks; the ``fc0`` input and its gradient, every tail layer's
    pre-activation and activation, and two gradient buffers as wide as the widest tail layer.  Once per workgroup, where ``emb_dim`` is at
    most ``STAGE_EMB``: the GRU's two kernels and its bias, the AUGRU's nine kernels and six biases (``15 D D + 12 D``); other widths read
    them from L2."""
    T, D, H = fam.hist_len, fam.emb_dim, fam.att_hidden
    per = (T + 1) * D + 21 * T * D + 2 * T * H + 2 * T + 8 * D + 2 * fam.fan0 + 2 * sum(fam.hidden) + 2 * max(fam.hidden)
    once = 15 * D * D + 12 * D if D <= STAGE_EMB else 0
    return 4 * (int(tile) * per + once)


# ---------------------------------------------------------------- the definition

def tanh_def(z):
    """``(s + s) - 1`` with ``s = sigmoid_def(z + z)``."""
    z = np.asarray(z, dtype=_F)
    with np.errstate(all="ignore"):
        s = sigmoid_def(z + z)
        return ((s + s) - _F(1.0)).astype(_F)


def _matmul(x, W):
    """``x @ W`` in ``_dense``'s ``k`` order from ``+0``, without a bias."""
    z = np.zeros((x.shape[0], W.shape[1]), dtype=_F)
    for k in range(W.shape[0]):
        z = z + x[:, k:k + 1] * W[k][None, :]
    return z


def forward_host(fam: DienFamily, w, ids, dense, keep: Optional[dict] = None):
    """The definition's probabilities ``[n]`` for packed rows; ``keep`` (a dict) receives every intermediate the backward pass reads."""
    ids, dense = np.asarray(ids, dtype=np.int32), np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, T, D, H = ids.shape[0], fam.hist_len, fam.emb_dim, fam.att_hidden
    one = _F(1.0)
    with np.errstate(all="ignore"):
        rows = [_rows(w[fam.tables[fam.table_of[c]]], ids[:, c]) for c in range(len(fam.columns))]
        c = rows[0]
        x = np.stack(rows[1:T + 1], axis=1).reshape(n, T, D)
        mask = ids[:, 1:T + 1] != 0
        # ---- the GRU
        Wk, Uk, bk = w["gru/kernel"], w["gru_rec/kernel"], w["gru/bias"]
        h, out = np.zeros((n, D), dtype=_F), np.zeros((n, D), dtype=_F)
        hp, gz, gr, ghh, gmh, g = (np.zeros((n, T, D), dtype=_F) for _ in range(6))
        for t in range(T):
            mx, mh = _dense(x[:, t], Wk, bk[0]), _dense(h, Uk, bk[1])
            z = sigmoid_def(mx[:, :D] + mh[:, :D])
            r = sigmoid_def(mx[:, D:2 * D] + mh[:, D:2 * D])
            hh = tanh_def(mx[:, 2 * D:] + r * mh[:, 2 * D:])
            hn = (z * h + (one - z) * hh).astype(_F)
            hp[:, t], gz[:, t], gr[:, t], ghh[:, t], gmh[:, t] = h, z, r, hh, mh[:, 2 * D:]
            m = mask[:, t, None]
            h, out = np.where(m, hn, h), np.where(m, hn, out)
            g[:, t] = out
        # ---- the attention gate
        q = (g * c[:, None, :]).astype(_F)
        y = sigmoid_def(_dense(q.reshape(n * T, D), w["att0/kernel"], w["att0/bias"])).reshape(n, T, H)
        a = sigmoid_def(_dense(y.reshape(n * T, H), w["att1/kernel"], w["att1/bias"])[:, 0]).reshape(n, T)
        # ---- the AUGRU
        hs = np.broadcast_to(w["augru/h0"].reshape(1, D), (n, D)).astype(_F)
        hsp, rt, zt, hc = (np.zeros((n, T, D), dtype=_F) for _ in range(4))
        pre = np.zeros((n, T, 3, D), dtype=_F)

        def gate(k, name, gt, hid, t):
            pre[:, t, k] = _dense(gt, w["augru_%s_in/kernel" % name], w["augru_%s_in/bias" % name]) + _matmul(hid, w["augru_%s_hid/kernel" % name])
            return _dense(pre[:, t, k], w["augru_%s_out/kernel" % name], w["augru_%s_out/bias" % name])
        for t in range(T):
            hsp[:, t] = hs
            rt[:, t] = sigmoid_def(gate(0, "r", g[:, t], hs, t))
            zt[:, t] = sigmoid_def(gate(1, "z", g[:, t], hs, t))
            hc[:, t] = tanh_def(gate(2, "h", g[:, t], (hs * zt[:, t]).astype(_F), t))
            u = (a[:, t, None] * rt[:, t]).astype(_F)
            hs = ((one - u) * hs + u * hc[:, t]).astype(_F)
        # ---- the tail and the head
        x0 = np.zeros((n, fam.fan0), dtype=_F)
        for k, (src, sub) in enumerate(zip(fam.xsrc, fam.xsub)):
            x0[:, k] = dense[:, sub] if src == SRC_NUMERIC else hs[:, sub] if src == SRC_POOLED else rows[src][:, sub]
        acts, zs = [x0], []
        for i in range(len(fam.hidden)):
            z = _dense(acts[-1], w["fc%d/kernel" % i], w["fc%d/bias" % i])
            zs.append(z)
            acts.append(prelu(z, w["fc%d_prelu/alpha" % i][None]))
        logit = _dense(acts[-1], w["head/kernel"], w["head/bias"])[:, 0]
        p = sigmoid_def(logit)
    if keep is not None:
        keep.update(c=c, x=x, mask=mask, hp=hp, gz=gz, gr=gr, ghh=ghh, gmh=gmh, g=g, q=q, y=y, a=a, hsp=hsp, rt=rt, zt=zt, hc=hc, pre=pre, hs=hs,
                    acts=acts, zs=zs, logit=logit)
    return p


def step_gradients(fam: DienFamily, w, ids, dense, labels, tile: Optional[int] = None, keep: Optional[dict] = None):
    """One step's gradients: ``({name: gradient}, p)`` for the batch ``(ids, dense, labels)`` under the weights ``w``; ``keep`` receives
    the forward's intermediates, ``dg [n, T, D]`` and the per-``(sample, column)`` row gradients ``drow [n, C, D]``."""
    ids, labels = np.asarray(ids, dtype=np.int32), np.asarray(labels, dtype=_F)
    dense = np.asarray(dense, dtype=_F).reshape(len(ids), fam.n_dense)
    n, tile = ids.shape[0], default_tile(fam) if tile is None else int(tile)
    T, D, H, L, C = fam.hist_len, fam.emb_dim, fam.att_hidden, len(fam.hidden), len(fam.columns)
    one = _F(1.0)
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
        dhs = dx[:, col_rows(SRC_POOLED)]
        c, gg, a, y = k_["c"], k_["g"], k_["a"], k_["y"]
        # ---- the AUGRU, from the last slot down
        do3, dpre3 = np.zeros((n, T, 3, D), dtype=_F), np.zeros((n, T, 3, D), dtype=_F)
        da = np.zeros((n, T), dtype=_F)
        hid3 = np.zeros((n, T, 3, D), dtype=_F)                                  # the three gates' ``hid`` inputs: hs, hs, hs z_t
        ker = lambda name, gate: w["augru_%s_%s/kernel" % (gate, name)]
        for t in range(T - 1, -1, -1):
            hs, r, z, hc = k_["hsp"][:, t], k_["rt"][:, t], k_["zt"][:, t], k_["hc"][:, t]
            u = (a[:, t, None] * r).astype(_F)
            du, dhc = dhs * (hc - hs), dhs * u
            s = np.zeros(n, dtype=_F)
            for d in range(D):
                s = s + du[:, d] * r[:, d]
            da[:, t] = s
            dr = du * a[:, t, None]
            do_h = dhc * (one - hc * hc)
            dpre_h = _back(ker("out", "h"), do_h)
            dhz = _back(ker("hid", "h"), dpre_h)
            dzt = dhz * hs
            do_z, do_r = (dzt * z) * (one - z), (dr * r) * (one - r)
            dpre_z, dpre_r = _back(ker("out", "z"), do_z), _back(ker("out", "r"), do_r)
            do3[:, t, 0], do3[:, t, 1], do3[:, t, 2] = do_r, do_z, do_h
            dpre3[:, t, 0], dpre3[:, t, 1], dpre3[:, t, 2] = dpre_r, dpre_z, dpre_h
            hid3[:, t, 0], hid3[:, t, 1], hid3[:, t, 2] = hs, hs, (hs * z).astype(_F)
            dhs = ((dhs * (one - u) + _back(ker("hid", "r"), dpre_r)) + _back(ker("hid", "z"), dpre_z)) + dhz * z
        g["augru/h0"] = _grad_bias(dhs, tile).reshape(1, D)
        pairs = lambda v: v.reshape(n * T, -1)
        for k, name in enumerate(GATES):
            g["augru_%s_in/kernel" % name] = _grad_kernel(pairs(gg), pairs(dpre3[:, :, k]), tile * T)
            g["augru_%s_in/bias" % name] = _grad_bias(pairs(dpre3[:, :, k]), tile * T)
            g["augru_%s_hid/kernel" % name] = _grad_kernel(pairs(hid3[:, :, k]), pairs(dpre3[:, :, k]), tile * T)
            g["augru_%s_out/kernel" % name] = _grad_kernel(pairs(k_["pre"][:, :, k]), pairs(do3[:, :, k]), tile * T)
            g["augru_%s_out/bias" % name] = _grad_bias(pairs(do3[:, :, k]), tile * T)
        # ---- the attention gate
        dl = ((da * a) * (one - a)).astype(_F).reshape(n * T, 1)
        g["att1/kernel"], g["att1/bias"] = _grad_kernel(pairs(y), dl, tile * T), _grad_bias(dl, tile * T)
        dyy = _back(w["att1/kernel"], dl)
        de = ((dyy * pairs(y)) * (one - pairs(y))).astype(_F)
        g["att0/kernel"], g["att0/bias"] = _grad_kernel(pairs(k_["q"]), de, tile * T), _grad_bias(de, tile * T)
        dq = _back(w["att0/kernel"], de).reshape(n, T, D)
        dg =np.zeros((n, T, D), dtype=_F)
        for t in range(T):
            dg[:, t] = ((dq[:, t] * c + _back(ker("in", "r"), dpre3[:, t, 0])) + _back(ker("in", "z"), dpre3[:, t, 1])) + _back(ker("in", "h"), dpre3[:, t, 2])
        drow = np.zeros((n, C, D), dtype=_F)
        for cc in range(C):
            ks = col_rows(cc)
            if len(ks) == D:
                drow[:, cc] = dx[:, ks]
        xc = drow[:, 0].copy()
        for t in range(T):
            xc = xc + dq[:, t] * gg[:, t]
        drow[:, 0] = xc
        # ---- the masked GRU, from the last slot down
        dmx, dmh = np.zeros((n, T, 3 * D), dtype=_F), np.zeros((n, T, 3 * D), dtype=_F)
        dh, do = np.zeros((n, D), dtype=_F), np.zeros((n, D), dtype=_F)
        zero = np.zeros((n, D), dtype=_F)
        for t in range(T - 1, -1, -1):
            m = k_["mask"][:, t, None]
            h, z, r, hh, mhh = k_["hp"][:, t], k_["gz"][:, t], k_["gr"][:, t], k_["ghh"][:, t], k_["gmh"][:, t]
            do = do + dg[:, t]
            dhn = dh + do
            dzg, dhh = dhn * (h - hh), dhn * (one - z)
            dp_h = dhh * (one - hh * hh)
            drr = dp_h * mhh
            dp_z, dp_r = (dzg * z) * (one - z), (drr * r) * (one - r)
            dmx[:, t] = np.where(m, np.concatenate([dp_z, dp_r, dp_h], axis=1), _F(0.0))
            dmh[:, t] = np.where(m, np.concatenate([dp_z, dp_r, dp_h * r], axis=1), _F(0.0))
            drow[:, 1 + t] = np.where(m, _back(w["gru/kernel"], dmx[:, t]), _F(0.0))
            dh = np.where(m, dhn * z + _back(w["gru_rec/kernel"], dmh[:, t]), dh).astype(_F)
            do = np.where(m, zero, do)
        g["gru/kernel"] = _grad_kernel(pairs(k_["x"]), pairs(dmx), tile * T)
        g["gru_rec/kernel"] = _grad_kernel(pairs(k_["hp"]), pairs(dmh), tile * T)
        g["gru/bias"] = np.stack([_grad_bias(pairs(dmx), tile * T), _grad_bias(pairs(dmh), tile * T)])
        for t, name in enumerate(fam.tables):
            cs = [cc for cc in range(C) if fam.table_of[cc] == t]
            g[name] = _grad_rows(ids[:, cs], drow[:, cs], _table_vocab(fam, t), tile)
    if keep is not None:
        keep.update(k_, dx=dx, drow=drow, dg=dg, dq=dq, da=da, dmx=dmx, dmh=dmh)
    return g, p


def validate_host(fam: DienFamily, ids, dense, labels):
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


def train_host(fam: DienFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
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
    s = L.TrainDienModel()
    s.n_cols, s.n_dense, s.emb_dim, s.hist_len, s.att_hidden, s.n_x, s.n_layers = (len(fam.columns), fam.n_dense, fam.emb_dim, fam.hist_len, fam.att_hidden,
                                                                                  fam.fan0, len(fam.hidden))
    for c, (_, kind, vocab) in enumerate(fam.columns):
        s.vocab[c], s.genre[c], s.table[c] = vocab, 1 if kind == "genre" else 0, fam.table_of[c]
    for i, h in enumerate(fam.hidden):
        s.width[i] = h
    for k, (src, sub) in enumerate(zip(fam.xsrc, fam.xsub)):
        s.xsrc[k], s.xsub[k] = src, sub
    return s


def train_device(fam: DienFamily, weights, ids, dense, labels, batch_size: int = DEFAULT_BATCH, epochs: int = 5, learning_rate: float = 0.001,
                 order=None, tile: Optional[int] = None, state=None, device=None, workspace=None, num_thresholds: int = 200) -> TrainResult:
    """:func:`train_host` on the device (``sprk_train_dien_fit``): the same bits in every weight, ``m``, ``v`` and ``p``; the history through
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
        need = int(lib.sprk_train_dien_workspace_bytes(C.byref(ms), N, B, tile))
        if workspace is None:
            workspace = torch.empty(max(need, 16) // 8 + 2, dtype=torch.int64, device=dev)
        c1, c2, eps = adam_constants()
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if E and N:
            L.check(lib.sprk_train_dien_fit(C.byref(ms), ptr(ids), ptr(dense) if fam.n_dense else None, ptr(labels), ptr(order_t) if order is not None else None,
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
    """``CTRModel.fit`` for a ``DIEN``: the same arguments (a dict of columns with ``"label"`` or ``y``, or an iterable of ``(features,
    labels)`` batches) and the same return value (per epoch ``[loss, accuracy, roc_auc, pr_auc]``); the trained weights are set on
    ``model`` and Adam's moments kept in ``model._fit_state``, so a second call continues.  This function is the entry: ``DIEN.fit``
    itself still raises ``NotImplementedError``, as ``DIN.fit`` does."""
    import sys
    fam = family_of(model)
    return model._fit_with(sys.modules[__name__], fam, x, y, batch_size, epochs, learning_rate, order, tile)
