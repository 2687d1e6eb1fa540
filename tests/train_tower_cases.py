"""Shared cases of tests/test_train_tower.py (the two-tower NeuralCF trainer's definition against independent implementations, no GPU) and
tests/test_gpu_train_tower.py (``trainer_tower.train_device`` / ``tower_rows_device`` / ``towers`` against their host definitions, byte for
byte): small families over tiny vocabularies, weights, data, the torch restatement of the graph and the data of the learning test."""
import numpy as np

from sparrowrecsys_amd import trainer_tower as TT
from tests import train_cases as TC

F = np.float32
same_bits = TC.same_bits


def family(movies=7, users=5, emb_dim=3, hidden=(5, 4)):
    return TT.make_family(movies, users, emb_dim, hidden)


def weights(fam, seed=0, scale=1.0):
    """Glorot-sized tower kernels, biases in [0, 0.2) (so that both towers have live units), table rows of unit scale, the head's kernel of
    magnitude 0.5 .. 1.5 with the seed's sign."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shape in TT.param_shapes(fam).items():
        if k.startswith("emb/"):
            w[k] = (rng.standard_normal(shape) / np.sqrt(shape[1]) * scale).astype(F)
        elif k == "head/kernel":
            w[k] = (np.array([[rng.uniform(0.5, 1.5) * (1 if seed % 2 == 0 else -1)]]) * scale).astype(F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            w[k] = (rng.uniform(-lim, lim, size=shape) * scale).astype(F)
        else:
            w[k] = (rng.uniform(0.0, 0.2, size=shape) * scale).astype(F)
    return w


def data(fam, n, seed=0):
    """``(ids [n, 2] int32, dense [n, 0] float32, labels [n] float32)``: ids uniform over the vocabularies, labels fair coins."""
    rng = np.random.default_rng(seed + 1000)
    ids = np.stack([rng.integers(0, v, size=n) for _, _, v in fam.columns], axis=1).astype(np.int32)
    return ids, np.zeros((n, 0), dtype=F), (rng.random(n) < 0.5).astype(F)


def small(n, seed=0, **kw):
    """-> ``(fam, weights, ids, dense, labels)``; the knobs are ``family``'s: movies, users, emb_dim, hidden."""
    fam = family(**kw)
    return (fam, weights(fam, seed)) + data(fam, n, seed)


def dense_floats(fam):
    """The items of the Dense Adam kernel's loop: both towers' layers and the head."""
    s = TT.param_shapes(fam)
    return sum(int(np.prod(s[k])) for k in s if not k.startswith("emb/"))


def table_floats(fam):
    return sum(v for _, _, v in fam.columns) * fam.emb_dim


def flat(fam, d):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in TT.param_names(fam)])


def torch_logit(fam, p, ids):
    """The graph in torch from a dict of tensors ``p``: -> the logit ``[n]``."""
    import torch
    import torch.nn.functional as Fn
    ids_t = torch.from_numpy(np.asarray(ids, dtype=np.int64))
    out = []
    for c, side in enumerate(("item", "user")):
        a = Fn.embedding(ids_t[:, c], p["emb/" + fam.columns[c][0]])
        for i in range(len(fam.hidden)):
            a = Fn.relu(Fn.linear(a, p["%s%d/kernel" % (side, i)].t(), p["%s%d/bias" % (side, i)]))
        out.append(a)
    dot = (out[0] * out[1]).sum(dim=1, keepdim=True)
    return Fn.linear(dot, p["head/kernel"].t(), p["head/bias"])[:, 0]


def torch_gradients(fam, w, ids, labels, dtype):
    """Mean binary cross-entropy through the logit, autograd in ``dtype`` on the CPU.  -> ``({name: gradient as float64 numpy}, p)``."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad=True) for k, v in w.items()}
    logit = torch_logit(fam, p, ids)
    Fn.binary_cross_entropy_with_logits(logit, torch.tensor(np.asarray(labels, dtype=np.float64), dtype=dtype), reduction="mean").backward()
    return {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}, torch.sigmoid(logit).detach().numpy()


def torch_sample_terms(fam, w, ids, labels, name):
    """The float64 run's terms of one tensor's gradient: ``[n, *shape]``, sample ``i``'s own contribution ``d(loss_i / n) / d tensor``."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    each = Fn.binary_cross_entropy_with_logits(torch_logit(fam, p, ids), torch.tensor(np.asarray(labels, dtype=np.float64)), reduction="none") / len(labels)
    return np.stack([torch.autograd.grad(each[i], p[name], retain_graph=True)[0].numpy() for i in range(len(labels))])


def float64_gradients(fam, w, ids, labels):
    """The definition restated in float64 with plain numpy sums (no tiles, no fixed order): ``({name: gradient}, p)``."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    ids, y = np.asarray(ids), np.asarray(labels, dtype=np.float64)
    n, L = len(y), len(fam.hidden)
    acts = {}
    for c, side in enumerate(("item", "user")):
        acts[side] = [w["emb/" + fam.columns[c][0]][ids[:, c]]]
        for i in range(L):
            acts[side].append(np.maximum(acts[side][-1] @ w["%s%d/kernel" % (side, i)] + w["%s%d/bias" % (side, i)], 0.0))
    dot = (acts["item"][L] * acts["user"][L]).sum(axis=1)
    hk = w["head/kernel"][0, 0]
    p = 1.0 / (1.0 + np.exp(-(dot * hk + w["head/bias"][0])))
    dl = (p - y) / n
    g = {"head/kernel": np.array([[(dot * dl).sum()]]), "head/bias": np.array([dl.sum()])}
    for c, (side, other) in enumerate((("item", "user"), ("user", "item"))):
        dz = np.where(acts[side][L] > 0, (dl * hk)[:, None] * acts[other][L], 0.0)
        for i in range(L - 1, -1, -1):
            g["%s%d/kernel" % (side, i)], g["%s%d/bias" % (side, i)] = acts[side][i].T @ dz, dz.sum(axis=0)
            dz = dz @ w["%s%d/kernel" % (side, i)].T
            if i:
                dz = np.where(acts[side][i] > 0, dz, 0.0)
        out = np.zeros((fam.columns[c][2], fam.emb_dim))
        np.add.at(out, ids[:, c], dz)
        g["emb/" + fam.columns[c][0]] = out
    return g, p


# ---- the learning test: 12 movies and 12 users in 3 groups each, label = (movie's group == user's group): neither tower sees the other side's id, so
# ---- only the dot of the two towers' outputs can carry the label.  384 rows; one data seed.
LEARN_SEED, LEARN_IDS, LEARN_GROUPS, LEARN_ROWS = 2718, 12, 3, 384


def learning(seed=0, emb_dim=8, hidden=(16,)):
    """-> ``(fam, weights, ids, dense, labels)``; tables N(0, 0.5), Glorot kernels, biases 0.1, the head's kernel 1, from ``seed``."""
    fam = family(LEARN_IDS, LEARN_IDS, emb_dim, hidden)
    rng = np.random.default_rng(LEARN_SEED)
    ids = np.stack([rng.integers(0, LEARN_IDS, LEARN_ROWS), rng.integers(0, LEARN_IDS, LEARN_ROWS)], axis=1).astype(np.int32)
    y = (ids[:, 0] % LEARN_GROUPS == ids[:, 1] % LEARN_GROUPS).astype(F)
    init = np.random.default_rng(seed)
    w = {}
    for k, shape in TT.param_shapes(fam).items():
        if k.startswith("emb/"):
            w[k] = (init.standard_normal(shape) * 0.5).astype(F)
        elif k == "head/kernel":
            w[k] = np.ones(shape, dtype=F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            w[k] = init.uniform(-lim, lim, size=shape).astype(F)
        else:
            w[k] = np.full(shape, 0.1 if k != "head/bias" else 0.0, dtype=F)
    return fam, w, ids, np.zeros((LEARN_ROWS, 0), dtype=F), y


def auc(y, p):
    """The exact ROC AUC (ties count a half) of scores ``p`` for 0 / 1 labels ``y``."""
    y, p = np.asarray(y) > 0.5, np.asarray(p, dtype=np.float64)
    pos, neg = p[y], p[~y]
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg)))


def torch_adam_fit(fam, w, ids, y, batch, epochs, lr):
    """``torch.optim.Adam(eps=1e-7)`` on the float32 twin of the graph over the same arrays, batches in input order.  -> the training AUC of
    all rows under the final weights."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float32, requires_grad=True) for k, v in w.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr, eps=1e-7)
    yt = torch.from_numpy(y)
    for _ in range(epochs):
        for b0 in range(0, len(y), batch):
            opt.zero_grad()
            Fn.binary_cross_entropy_with_logits(torch_logit(fam, p, ids[b0:b0 + batch]), yt[b0:b0 + batch]).backward()
            opt.step()
    with torch.no_grad():
        return auc(y, torch_logit(fam, p, ids).numpy())


# ---- the end-to-end test's ratings: tests/train_wide_cases.py structured_ratings() (the movie says how a held-out rating goes)
def structured_ratings(seed=7, users=30, per_user=100):
    from tests import train_wide_cases as TWC
    return TWC.structured_ratings(seed, users, per_user)
