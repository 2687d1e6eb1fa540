"""Shared cases of tests/test_train_wide.py (the Wide&Deep trainer's definition against independent implementations, no GPU) and
tests/test_gpu_train_wide.py (``trainer_wide.train_device`` against ``train_host``, byte for byte): small ``WideNDeep`` models in both
cross forms, weights, data, the torch restatement of the graph and the data of the learning test."""
import numpy as np

from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer_wide as TW
from tests import train_cases as TC

F = np.float32
same_bits = TC.same_bits

REFERENCE_SHAPE = dict(emb_dim=10, hidden=(128, 128), movies=30, users=40, rated=30, cross_buckets=10000)


def model(emb_dim=3, hidden=(5,), movies=7, users=5, rated=7, cross_buckets=11, cross_dim=0, seed=0):
    """A ``WideNDeep`` over tiny vocabularies (the eight genre tables keep their 19 rows)."""
    return M.WideNDeep(seed=seed, emb_dim=emb_dim, hidden=hidden, movie_buckets=movies, user_buckets=users, rated_buckets=rated, cross_buckets=cross_buckets,
                       cross_dim=cross_dim)


def family(**kw):
    return TW.family_of(model(**kw))


def weights(fam, seed=0, scale=1.0):
    """Glorot-sized kernels (the head's from its deep fan: the indicator's 10 000 rows would shrink it to nothing), small biases, table rows of
    unit scale."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shape in TW.param_shapes(fam).items():
        if k.startswith("emb/"):
            w[k] = (rng.standard_normal(shape) / np.sqrt(shape[1]) * scale).astype(F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / ((fam.widths[-1] if k == "head/kernel" else shape[0]) + shape[1]))
            w[k] = (rng.uniform(-lim, lim, size=shape) * scale).astype(F)
        else:
            w[k] = (rng.uniform(-0.1, 0.1, size=shape) * scale).astype(F)
    return w


def data(fam, n, seed=0, none_rate=0.25):
    """``train_cases.data`` over the eleven columns: ids uniform, genre columns -1 at ``none_rate``, numerics standard normal, labels fair coins."""
    return TC.data(fam, n, seed, none_rate)


def small(n, seed=0, **kw):
    fam = family(**kw)
    return (fam, weights(fam, seed)) + data(fam, n, seed)


def dense_floats(fam):
    """The items of ``k_tr_dense_adam``'s loop: the hidden layers, ``head/bias`` and ``head/kernel[:H + cross_dim]``."""
    s = TW.param_shapes(fam)
    return sum(int(np.prod(s[name + "/kernel"])) + int(np.prod(s[name + "/bias"])) for name in fam.layers[:-1]) + 1 + fam.widths[-1] + fam.cross_dim


def table_floats(fam):
    """The items of ``k_tr_table_adam``'s loop: the floats of the ten deep tables."""
    s = TW.param_shapes(fam)
    return sum(int(np.prod(s[t])) for t in fam.tables)


def cross_floats(fam):
    """The items of ``k_trw_cross_adam``'s loop: ``cross_buckets`` rows of ``max(1, cross_dim)`` floats."""
    return fam.cross_buckets * max(1, fam.cross_dim)


def cross_pairs(fam):
    """Every ``(movieId, userRatedMovie1)`` pair of the two vocabularies with its bucket: -> ``(a, b, bucket)``, flat arrays."""
    a, b = np.meshgrid(np.arange(fam.columns[fam.cross_a][2]), np.arange(fam.columns[fam.cross_b][2]), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    return a, b, TW.cross_bucket_host(a, b, fam.cross_buckets)


def torch_logit(fam, p, ids, dn, dtype):
    """The graph in torch from a dict of tensors ``p``: -> the logit ``[n]``; the bucket from ``oracle.ctr_oracle.crossed_bucket_np``."""
    import torch
    import torch.nn.functional as Fn
    from oracle import ctr_oracle as O
    ids_t = torch.from_numpy(np.asarray(ids, dtype=np.int64))
    bucket = torch.from_numpy(O.crossed_bucket_np([ids[:, fam.cross_a], ids[:, fam.cross_b]], fam.cross_buckets))
    blocks = []
    for c, tab in enumerate(fam.tables):
        ok = (ids_t[:, c] >= 0).to(dtype)[:, None]
        blocks.append(Fn.embedding(ids_t[:, c].clamp(min=0), p[tab]) * ok)
    x = torch.stack([dn[:, s] if c < 0 else blocks[c][:, s] for c, s in zip(fam.xcol, fam.xsub)], dim=1)
    for name in fam.layers[:-1]:
        x = Fn.relu(Fn.linear(x, p[name + "/kernel"].t(), p[name + "/bias"]))
    H, hk = fam.widths[-1], p["head/kernel"]
    if fam.cross_dim:
        return Fn.linear(torch.cat([x, Fn.embedding(bucket, p["emb/cross"])], dim=1), hk.t(), p["head/bias"])[:, 0]
    return Fn.linear(x, hk[:H].t(), p["head/bias"])[:, 0] + hk[H + bucket, 0]


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


# ---- the learning test: the label is a fixed random function of the cross bucket (a Bernoulli of 0.9 or 0.1 by the bucket's coin), so only the
# ---- cross can carry it: movieId and userRatedMovie1 are uniform over 12 ids each, 144 pairs over 61 buckets; the deep side is shrunk to
# ---- hidden (2,), emb_dim 2, constant numerics, and every other id column is constant.  2 048 rows; one data seed.
LEARN_SEED, LEARN_MOVIES, LEARN_BUCKETS, LEARN_ROWS = 2718, 12, 61, 2048


def learning(cross_dim=0, seed=0):
    """-> ``(fam, weights, ids, dense, labels)``: the reference initialisers from ``seed``."""
    mo = model(emb_dim=2, hidden=(2,), movies=LEARN_MOVIES, users=3, rated=LEARN_MOVIES, cross_buckets=LEARN_BUCKETS, cross_dim=cross_dim, seed=seed)
    mo.set_weights(mo.init_weights(seed, trained_like=False))
    fam = TW.family_of(mo)
    rng = np.random.default_rng(LEARN_SEED)
    ids = np.zeros((LEARN_ROWS, len(fam.columns)), dtype=np.int32)
    ids[:, fam.cross_a], ids[:, fam.cross_b] = rng.integers(0, LEARN_MOVIES, LEARN_ROWS), rng.integers(0, LEARN_MOVIES, LEARN_ROWS)
    coin = rng.random(LEARN_BUCKETS) < 0.5
    y = (rng.random(LEARN_ROWS) < np.where(coin[TW.buckets_of(fam, ids)], 0.9, 0.1)).astype(F)
    return fam, {k: np.array(v, dtype=F) for k, v in mo.weights.items()}, ids, np.ones((LEARN_ROWS, fam.n_dense), dtype=F), y


def torch_adam_fit(fam, w, ids, dense, y, batch, epochs, lr):
    """``torch.optim.Adam(eps=1e-7)`` on the float32 twin of the graph over the same arrays, batches in input order.  -> the final mean
    training loss (over all rows, under the final weights)."""
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
        return float(Fn.binary_cross_entropy_with_logits(torch_logit(fam, p, ids, dn, torch.float32), yt))


# ---- the end-to-end test's ratings: 30 users x 100 ratings of tests/featureeng_cases.py's 58 movies with ids 1 .. 115; every other movie is liked
# ---- (a rating of 4 to 5 nine times in ten, else 1 to 2.5) and the others disliked likewise, so the movie -- its embedding, its average
# ---- rating -- says how a held-out rating goes; timestamps are distinct and shuffled among the users.
def structured_ratings(seed=7, users=30, per_user=100):
    rng = np.random.RandomState(seed)
    n = users * per_user
    movie = rng.choice(np.arange(1, 116, 2), n)
    liked = ((movie // 2) % 2 == 0) == (rng.random_sample(n) < 0.9)
    rating = np.where(liked, rng.randint(8, 11, n), rng.randint(2, 6, n)) / 2.0
    return {"userId": np.repeat(np.arange(1, users + 1), per_user).astype(np.int64), "movieId": movie.astype(np.int64), "rating": rating.astype(np.float64),
            "timestamp": (1_000_000 + rng.permutation(n)).astype(np.int64)}


def host_loss(fam, w, ids, dense, y):
    """Mean binary cross-entropy of ``forward_host`` under ``w``, in float64 with Keras' clip of 1e-7."""
    p = np.clip(TW.forward_host(fam, w, ids, dense).astype(np.float64), 1e-7, 1 - 1e-7)
    return float(-(y * np.log(p) + (1 - y) * np.log(1 - p)).mean())
