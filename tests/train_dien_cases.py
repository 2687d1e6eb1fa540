"""Shared cases of tests/test_train_dien.py (the DIEN trainer's definition against independent implementations, no GPU) and
tests/test_gpu_train_dien.py (``trainer_dien.train_device`` against ``train_host``, byte for byte): small ``DienFamily`` tuples built
directly (``models.DIEN`` itself only builds ``emb_dim`` 10 or 16 with ``att_hidden`` 32), weights, data with about a third of the history
ids 0, the float64 torch restatement of the graph (mask included) and the order-only data of the learning test."""
import numpy as np

from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer_dien as TE
from tests import train_cases as TC

F = np.float32
same_bits = TC.same_bits

REFERENCE_SHAPE = dict(hist_len=5, emb_dim=10, att_hidden=32, hidden=(128, 64), movies=30, users=40)
PROFILE_NUM, CONTEXT_NUM = M.DIN._PROFILE_NUM, M.DIN._CONTEXT_NUM
NUMERICS = sorted(PROFILE_NUM + CONTEXT_NUM)


def family(hist_len=3, emb_dim=3, att_hidden=5, hidden=(6, 4), movies=7, users=5, genres=19, others=True):
    """A ``DienFamily`` laid out as ``DIEN._fc_rows()`` lays the tail's input out: the AUGRU's state, the candidate, the profile block and
    the context block, each sorted by name; the seven numerics sorted by name, which is ``model.numeric_keys``.  ``others=False``: the candidate and the
    history only (no user and genre columns), which lets ``emb_dim`` reach 64 inside ``fc0``'s 256 input rows."""
    T, D = hist_len, emb_dim
    cols = [("movieId", "id", movies)] + [("userRatedMovie%d" % (t + 1), "id", movies) for t in range(T)]
    tables, table_of = ["emb/movie"], [0] * (T + 1)
    if others:
        cols += [("userId", "id", users), ("userGenre1", "genre", genres), ("movieGenre1", "genre", genres)]
        tables += ["emb/userId", "emb/userGenre1", "emb/movieGenre1"]
        table_of += [1, 2, 3]
    keys = [k for k, _, _ in cols]
    numerics = NUMERICS
    xsrc, xsub = [TE.SRC_POOLED] * D + [0] * D, list(range(D)) * 2
    for block, embs in ((PROFILE_NUM, ["userId", "userGenre1"]), (CONTEXT_NUM, ["movieGenre1"])):
        names = {k: None for k in block}
        names.update({k + "_embedding": k for k in embs if others})
        for name in sorted(names):
            if names[name] is None:
                xsrc.append(TE.SRC_NUMERIC)
                xsub.append(numerics.index(name))
            else:
                xsrc += [keys.index(names[name])] * D
                xsub += list(range(D))
    fam = TE.DienFamily(cols, tables, table_of, D, T, att_hidden, [int(h) for h in hidden], len(numerics), xsrc, xsub)
    TE._check_family(fam)
    return fam


def weights(fam, seed=0, scale=1.0):
    """Glorot-sized kernels, small biases, table rows and ``augru/h0`` of unit scale, PReLU slopes on both sides of zero."""
    rng = np.random.default_rng(seed)
    w = {}
    for k in TE.param_names(fam):
        shape = TE.param_shapes(fam)[k]
        if k.startswith("emb/") or k == "augru/h0":
            w[k] = (rng.standard_normal(shape) / np.sqrt(shape[1]) * scale).astype(F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            w[k] = (rng.uniform(-lim, lim, size=shape) * scale).astype(F)
        elif k.endswith("/alpha"):
            w[k] = (rng.uniform(-0.3, 0.5, size=shape) * scale).astype(F)
        else:
            w[k] = (rng.uniform(-0.1, 0.1, size=shape) * scale).astype(F)
    return w


def data(fam, n, seed=0, none_rate=0.25, masked=1.0 / 3.0):
    """``train_cases.data`` with the history ids set to 0 at the rate ``masked`` (``masked=0``: history ids from 1)."""
    ids, dense, y = TC.data(fam, n, seed, none_rate)
    T = fam.hist_len
    rng = np.random.default_rng(seed + 2000)
    movies = fam.columns[0][2]
    if movies > 1:
        ids[:, 1:T + 1] = rng.integers(1, movies, size=(n, T))
    ids[:, 1:T + 1][rng.random((n, T)) < masked] = 0
    return ids, dense, y


def small(n, seed=0, **kw):
    fam = family(**kw)
    return (fam, weights(fam, seed)) + data(fam, n, seed)


def dense_floats(fam):
    """The floats of every parameter that is no table: the items of ``k_tr_dense_adam``'s loop."""
    return sum(int(np.prod(s)) for k, s in TE.param_shapes(fam).items() if k not in fam.tables)


def table_floats(fam):
    """The floats of all tables: the items of ``k_td_table_adam``'s loop."""
    return sum(int(np.prod(s)) for k, s in TE.param_shapes(fam).items() if k in fam.tables)


def kept_entries(fam, ids):
    """The entries of the device's schedule (``te_entry`` in csrc/k_train_dien.h): every id from 0, less the history slots that hold 0."""
    ids = np.asarray(ids)
    T = fam.hist_len
    return int((ids >= 0).sum()) - int((ids[:, 1:T + 1] == 0).sum())


def features(fam, ids, dense):
    """The feature dict ``oracle.ctr_oracle.dien_forward`` takes, from packed rows of a family with the user and genre columns."""
    T = fam.hist_len
    f = {"movieId": ids[:, 0], "userRatedMovies": ids[:, 1:T + 1], "userId": ids[:, T + 1], "userGenre1": ids[:, T + 2].astype(np.int64),
         "movieGenre1": ids[:, T + 3].astype(np.int64)}                               # (resolved genre indices pass through the oracle's lookup)
    for j, k in enumerate(NUMERICS):
        f[k] = dense[:, j]
    return f


def torch_logit(fam, p, ids_t, dn, dtype, parts=None):
    """The graph in torch from a dict of tensors ``p``, the Keras mask included: -> the logit ``[n]``."""
    import torch
    import torch.nn.functional as Fn
    T, D = fam.hist_len, fam.emb_dim
    prelu = lambda z, al: Fn.relu(z) - al * Fn.relu(-z)
    rows = []
    for c in range(len(fam.columns)):
        ok = (ids_t[:, c] >= 0).to(dtype)[:, None]
        rows.append(Fn.embedding(ids_t[:, c].clamp(min=0), p[fam.tables[fam.table_of[c]]]) * ok)
    c = rows[0]
    n = c.shape[0]
    h = torch.zeros((n, D), dtype=dtype)
    out, gs = h, []
    for t in range(T):
        mx = rows[1 + t] @ p["gru/kernel"] + p["gru/bias"][0]
        mh = h @ p["gru_rec/kernel"] + p["gru/bias"][1]
        z = torch.sigmoid(mx[:, :D] + mh[:, :D])
        r = torch.sigmoid(mx[:, D:2 * D] + mh[:, D:2 * D])
        hh = torch.tanh(mx[:, 2 * D:] + r * mh[:, 2 * D:])
        hn = z * h + (1 - z) * hh
        m = (ids_t[:, 1 + t] != 0)[:, None]
        h, out = torch.where(m, hn, h), torch.where(m, hn, out)
        gs.append(out)
    g = torch.stack(gs, dim=1)
    a = torch.sigmoid((torch.sigmoid(g * c[:, None, :] @ p["att0/kernel"] + p["att0/bias"]) @ p["att1/kernel"])[:, :, 0] + p["att1/bias"][0])

    def gate(name, gt, hid, act):
        pre = gt @ p["augru_%s_in/kernel" % name] + p["augru_%s_in/bias" % name] + hid @ p["augru_%s_hid/kernel" % name]
        return act(pre @ p["augru_%s_out/kernel" % name] + p["augru_%s_out/bias" % name])
    hs = p["augru/h0"].reshape(1, D).expand(n, D)
    for t in range(T):
        r_t, z_t = gate("r", g[:, t], hs, torch.sigmoid), gate("z", g[:, t], hs, torch.sigmoid)
        hc = gate("h", g[:, t], hs * z_t, torch.tanh)
        u = a[:, t, None] * r_t
        hs = (1 - u) * hs + u * hc
    x = torch.stack([dn[:, sub] if src == TE.SRC_NUMERIC else hs[:, sub] if src == TE.SRC_POOLED else rows[src][:, sub]
                     for src, sub in zip(fam.xsrc, fam.xsub)], dim=1)
    for i in range(len(fam.hidden)):
        x = prelu(Fn.linear(x, p["fc%d/kernel" % i].t(), p["fc%d/bias" % i]), p["fc%d_prelu/alpha" % i][None])
    if parts is not None:
        parts.update(g=g, a=a, hs=hs)
    return Fn.linear(x, p["head/kernel"].t(), p["head/bias"])[:, 0]


def torch_gradients(fam, w, ids, dense, labels, dtype):
    """Mean binary cross-entropy through the logit, autograd in ``dtype`` on the CPU.  -> ``({name: gradient as float64 numpy}, p)``."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad=True) for k, v in w.items()}
    logit = torch_logit(fam, p, torch.from_numpy(np.asarray(ids, dtype=np.int64)), torch.tensor(np.asarray(dense, dtype=np.float64), dtype=dtype), dtype)
    loss = Fn.binary_cross_entropy_with_logits(logit, torch.tensor(np.asarray(labels, dtype=np.float64), dtype=dtype), reduction="mean")
    loss.backward()
    return {k: (v.grad.detach().numpy().astype(np.float64) if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}, torch.sigmoid(logit).detach().numpy()


# ---- the learning test: samples in pairs that hold the same two movies in the two orders, (a, b) with label 1 and (b, a) with label 0; the
# ---- candidate, the user, the genres and the numerics are the same within a pair.  Nothing but the order of the history separates the labels.
ORDER_SEED, ORDER_MOVIES, ORDER_PAIRS = 2718, 6, 48


def ordered_pairs():
    """-> ``(fam, ids [2 P, 6], dense [2 P, 7], labels [2 P])`` at T = 2."""
    fam = family(hist_len=2, emb_dim=4, att_hidden=5, hidden=(8,), movies=ORDER_MOVIES, users=3)
    rng = np.random.default_rng(ORDER_SEED)
    P = ORDER_PAIRS
    a = rng.integers(1, ORDER_MOVIES, size=P)
    b = 1 + (a - 1 + rng.integers(1, ORDER_MOVIES - 1, size=P)) % (ORDER_MOVIES - 1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    assert (lo != hi).all()
    base, dn, _ = TC.data(fam, P, ORDER_SEED)
    ids = np.repeat(base, 2, axis=0)
    ids[0::2, 1], ids[0::2, 2] = lo, hi
    ids[1::2, 1], ids[1::2, 2] = hi, lo
    return fam, ids.astype(np.int32), np.repeat(dn, 2, axis=0), np.tile(np.array([1.0, 0.0], dtype=F), P)


# ---- the end-to-end test: 39 users x 100 ratings of the synthetic movies (tests/featureeng_cases.py); every other movie is good, and a rating is
# ---- 4.5 with probability 0.9 for a good movie and 0.1 for a bad one, else 2.0.  The candidate's row and movieAvgRating carry the label.
RATINGS_SEED, RATINGS_USERS, RATINGS_EACH = 1618, 39, 100


def planted_ratings():
    rng = np.random.default_rng(RATINGS_SEED)
    n = RATINGS_USERS * RATINGS_EACH
    movie = rng.choice(np.arange(1, 116, 2), n)
    high = rng.random(n) < np.where((movie // 2) % 2 == 0, 0.9, 0.1)
    return {"userId": np.repeat(np.arange(1, RATINGS_USERS + 1), RATINGS_EACH).astype(np.int64), "movieId": movie.astype(np.int64),
            "rating": np.where(high, 4.5, 2.0), "timestamp": rng.integers(1_000_000, 1_100_000, n).astype(np.int64)}
