"""Shared cases of tests/test_train_pair.py (the pair-dot DeepFM trainer's definition against independent implementations, no GPU) and
tests/test_gpu_train_pair.py (``trainer_pair.train_device`` against ``train_host``, byte for byte): small families over tiny vocabularies,
weights, data, the torch restatement of the graph and the data of the learning test."""
import numpy as np

from sparrowrecsys_amd import trainer_pair as TP
from sparrowrecsys_amd.schema import NUMERIC_KEYS
from tests import train_cases as TC

F = np.float32
same_bits = TC.same_bits

FIELDS = [("movieId", "id", 7), ("userId", "id", 5), ("userGenre1", "genre", 4), ("movieGenre1", "genre", 3)]
PAIRS = [("movieId", "userId"), ("movieGenre1", "userGenre1"), ("movieGenre1", "userId"), ("movieId", "userGenre1")]      # the reference's four
SIX = [("movieId", "id", 7), ("userId", "id", 5), ("userRatedMovie1", "id", 7), ("userGenre1", "genre", 4), ("userGenre2", "genre", 4), ("movieGenre1", "genre", 3)]
SIX_PAIRS = [(a, b) for a in ("movieId", "movieGenre1") for b in ("userId", "userRatedMovie1", "userGenre1", "userGenre2")]   # config 2's eight
EIGHT = [("f%d" % i, "genre" if i % 3 == 2 else "id", 2 + i) for i in range(8)]                                             # 2 .. 9 rows
EIGHT_PAIRS = [("f%d" % a, "f%d" % b) for a in range(8) for b in range(a + 1, 8)]                                           # all 28


def family(fields=FIELDS, pairs=PAIRS, deep_emb=("movieId", "userId"), shared=False, emb_dim=3, hidden=(5,), n_dense=7):
    return TP.make_family(fields, pairs, deep_emb, shared, emb_dim, hidden, list(NUMERIC_KEYS[:n_dense]))


def weights(fam, seed=0, scale=1.0):
    """Glorot-sized kernels (the head's from its Dense tail: the first-order rows would shrink it), small biases, table rows of unit scale."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shape in TP.param_shapes(fam).items():
        if k.startswith("emb/") or k.startswith("deep_emb/"):
            w[k] = (rng.standard_normal(shape) / np.sqrt(shape[1]) * scale).astype(F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / ((len(fam.pairs) + fam.hidden[-1] if k == "head/kernel" else shape[0]) + shape[1]))
            w[k] = (rng.uniform(-lim, lim, size=shape) * scale).astype(F)
        else:
            w[k] = (rng.uniform(-0.1, 0.1, size=shape) * scale).astype(F)
    return w


def data(fam, n, seed=0, none_rate=0.25):
    """``train_cases.data`` over the fields: ids uniform, genre columns -1 at ``none_rate``, numerics standard normal, labels fair coins."""
    return TC.data(fam, n, seed, none_rate)


def small(n, seed=0, **kw):
    """-> ``(fam, weights, ids, dense, labels)``; the knobs are ``family``'s: fields, pairs, deep_emb, shared, emb_dim, hidden, n_dense."""
    fam = family(**kw)
    return (fam, weights(fam, seed)) + data(fam, n, seed)


def dense_floats(fam):
    """The items of ``k_tp_dense_adam``'s loop: the deep layers, ``head/bias`` and ``head/kernel``'s tail ``[pairs + last width]``."""
    s = TP.param_shapes(fam)
    return sum(int(np.prod(s[k])) for k in s if k.startswith("deep") and not k.startswith("deep_emb/")) + 1 + len(fam.pairs) + fam.hidden[-1]


def table_floats(fam):
    """The items of ``k_tp_table_adam``'s loop: the floats of ``emb/*`` and ``deep_emb/*`` and ``head/kernel``'s first-order rows."""
    s = TP.param_shapes(fam)
    return sum(int(np.prod(s[k])) for k in s if k.startswith("emb/") or k.startswith("deep_emb/")) + fam.fo_total


def torch_logit(fam, p, ids, dn, dtype):
    """The graph in torch from a dict of tensors ``p``: -> the logit ``[n]``."""
    import torch
    import torch.nn.functional as Fn
    ids_t = torch.from_numpy(np.asarray(ids, dtype=np.int64))
    ok = [(ids_t[:, f] >= 0).to(dtype)[:, None] for f in range(len(fam.fields))]
    rows = lambda name, f: Fn.embedding(ids_t[:, f].clamp(min=0), p[name]) * ok[f]
    e = [rows("emb/" + k, f) for f, (k, _, _) in enumerate(fam.fields)]
    deep = [rows(TP._deep_table(fam, j), c) for j, c in enumerate(fam.deep_cols)]
    x = torch.stack([dn[:, s] if j < 0 else deep[j][:, s] for j, s in zip(fam.xsrc, fam.xsub)], dim=1)
    for i in range(len(fam.hidden)):
        x = Fn.relu(Fn.linear(x, p["deep%d/kernel" % i].t(), p["deep%d/bias" % i]))
    hk, T = p["head/kernel"], fam.fo_total
    first = sum(hk[fam.fo_off[f] + ids_t[:, f].clamp(min=0), 0] * ok[f][:, 0] for f in range(len(fam.fields)))
    dots = torch.stack([(e[a] * e[b]).sum(dim=1) for a, b in fam.pairs], dim=1)
    return first + Fn.linear(torch.cat([dots, x], dim=1), hk[T:].t(), p["head/bias"])[:, 0]


def torch_gradients(fam, w, ids, dense, labels, dtype):
    """Mean binary cross-entropy through the logit, autograd in ``dtype`` on the CPU.  -> ``({name: gradient as float64 numpy}, p)``."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad=True) for k, v in w.items()}
    logit = torch_logit(fam, p, np.asarray(ids), torch.tensor(np.asarray(dense, dtype=np.float64), dtype=dtype), dtype)
    loss = Fn.binary_cross_entropy_with_logits(logit, torch.tensor(np.asarray(labels, dtype=np.float64), dtype=dtype), reduction="mean")
    loss.backward()
    return {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}, torch.sigmoid(logit).detach().numpy()


def torch_sample_terms(fam, w, ids, dense, labels, name):
    """The float64 run's terms of one tensor's gradient: ``[n, *shape]``, sample ``i``'s own contribution ``d(loss_i / n) / d tensor``."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    logit = torch_logit(fam, p, np.asarray(ids), torch.tensor(np.asarray(dense, dtype=np.float64)), torch.float64)
    each = Fn.binary_cross_entropy_with_logits(logit, torch.tensor(np.asarray(labels, dtype=np.float64)), reduction="none") / len(labels)
    return np.stack([torch.autograd.grad(each[i], p[name], retain_graph=True)[0].numpy() for i in range(len(labels))])


def float64_gradients(fam, w, ids, dense, labels):
    """The definition restated in float64 with plain numpy sums (no tiles, no fixed order): ``({name: gradient}, p)``."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    ids, dense, y = np.asarray(ids), np.asarray(dense, dtype=np.float64), np.asarray(labels, dtype=np.float64)
    n, D, T, P = len(y), fam.emb_dim, fam.fo_total, len(fam.pairs)
    rows = lambda name, f: np.where((ids[:, f] >= 0)[:, None], w[name][np.maximum(ids[:, f], 0)], 0.0)
    e = [rows("emb/" + k, f) for f, (k, _, _) in enumerate(fam.fields)]
    deep = [rows(TP._deep_table(fam, j), c) for j, c in enumerate(fam.deep_cols)]
    x = np.stack([dense[:, s] if j < 0 else deep[j][:, s] for j, s in zip(fam.xsrc, fam.xsub)], axis=1)
    acts = [x]
    for i in range(len(fam.hidden)):
        acts.append(np.maximum(acts[-1] @ w["deep%d/kernel" % i] + w["deep%d/bias" % i], 0.0))
    dots = np.stack([(e[a] * e[b]).sum(axis=1) for a, b in fam.pairs], axis=1)
    hk = w["head/kernel"][:, 0]
    first = sum(np.where(ids[:, f] >= 0, hk[fam.fo_off[f] + np.maximum(ids[:, f], 0)], 0.0) for f in range(len(fam.fields)))
    cat = np.concatenate([dots, acts[-1]], axis=1)
    p = 1.0 / (1.0 + np.exp(-(first + cat @ hk[T:] + w["head/bias"][0])))
    dl = (p - y) / n
    g = {"head/bias": np.array([dl.sum()]), "head/kernel": np.zeros((len(hk), 1))}
    g["head/kernel"][T:, 0] = cat.T @ dl
    for f in range(len(fam.fields)):
        have = ids[:, f] >= 0
        np.add.at(g["head/kernel"][:, 0], fam.fo_off[f] + ids[have, f], dl[have])
    dz = np.where(acts[-1] > 0, dl[:, None] * hk[None, T + P:], 0.0)
    for i in range(len(fam.hidden) - 1, -1, -1):
        g["deep%d/kernel" % i], g["deep%d/bias" % i] = acts[i].T @ dz, dz.sum(axis=0)
        dz = dz @ w["deep%d/kernel" % i].T
        if i:
            dz = np.where(acts[i] > 0, dz, 0.0)
    de = [np.zeros((n, D)) for _ in fam.fields]
    for q, (a, b) in enumerate(fam.pairs):
        t = (dl * hk[T + q])[:, None]
        de[a] = de[a] + t * e[b]
        de[b] = de[b] + t * e[a]

    def table(f, d):
        out, have = np.zeros((fam.fields[f][2], D)), ids[:, f] >= 0
        np.add.at(out, ids[have, f], d[have])
        return out
    for j, c in enumerate(fam.deep_cols):
        dx = dz[:, TP._deep_rows_of(fam, j)]
        if fam.shared:
            de[c] = de[c] + dx
        else:
            g[TP._deep_table(fam, j)] = table(c, dx)
    for f, (k, _, _) in enumerate(fam.fields):
        g["emb/" + k] = table(f, de[f])
    return g, p


# ---- the learning test: label = (movieId + userId) mod 2 over 8 movies and 8 users, constant numerics, deep_emb on a third field that the label
# ---- ignores: the first order is additive in the two ids and the deep part never sees them, so only the dot <e_movie, e_user> can carry the
# ---- label.  256 rows; one data seed.
LEARN_SEED, LEARN_IDS, LEARN_ROWS = 1618, 8, 256
LEARN_FIELDS = [("movieId", "id", LEARN_IDS), ("userId", "id", LEARN_IDS), ("userRatedMovie1", "id", 3)]


def learning(seed=0, emb_dim=4):
    """-> ``(fam, weights, ids, dense, labels)``; tables N(0, 0.5), Glorot kernels, zero biases, from ``seed``."""
    fam = family(fields=LEARN_FIELDS, pairs=[("movieId", "userId")], deep_emb=("userRatedMovie1",), emb_dim=emb_dim, hidden=(4,), n_dense=2)
    rng = np.random.default_rng(LEARN_SEED)
    ids = np.stack([rng.integers(0, LEARN_IDS, LEARN_ROWS), rng.integers(0, LEARN_IDS, LEARN_ROWS), rng.integers(0, 3, LEARN_ROWS)], axis=1).astype(np.int32)
    y = ((ids[:, 0] + ids[:, 1]) % 2).astype(F)
    init = np.random.default_rng(seed)
    w = {}
    for k, shape in TP.param_shapes(fam).items():
        if "emb/" in k:
            w[k] = (init.standard_normal(shape) * 0.5).astype(F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / ((1 + fam.hidden[-1] if k == "head/kernel" else shape[0]) + shape[1]))
            w[k] = init.uniform(-lim, lim, size=shape).astype(F)
        else:
            w[k] = np.zeros(shape, dtype=F)
    return fam, w, ids, np.ones((LEARN_ROWS, fam.n_dense), dtype=F), y


def auc(y, p):
    """The exact ROC AUC (ties count a half) of scores ``p`` for 0 / 1 labels ``y``."""
    y, p = np.asarray(y) > 0.5, np.asarray(p, dtype=np.float64)
    pos, neg = p[y], p[~y]
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg)))


def torch_adam_fit(fam, w, ids, dense, y, batch, epochs, lr):
    """``torch.optim.Adam(eps=1e-7)`` on the float32 twin of the graph over the same arrays, batches in input order.  -> the training AUC of
    all rows under the final weights."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float32, requires_grad=True) for k, v in w.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr, eps=1e-7)
    dn, yt = torch.from_numpy(dense), torch.from_numpy(y)
    for _ in range(epochs):
        for b0 in range(0, len(y), batch):
            opt.zero_grad()
            Fn.binary_cross_entropy_with_logits(torch_logit(fam, p, ids[b0:b0 + batch], dn[b0:b0 + batch], torch.float32), yt[b0:b0 + batch]).backward()
            opt.step()
    with torch.no_grad():
        return auc(y, torch_logit(fam, p, ids, dn, torch.float32).numpy())


# ---- the end-to-end test's ratings: tests/train_wide_cases.py structured_ratings() (the movie says how a held-out rating goes)
def structured_ratings(seed=7, users=30, per_user=100):
    from tests import train_wide_cases as TWC
    return TWC.structured_ratings(seed, users, per_user)
