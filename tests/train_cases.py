"""Shared cases of tests/test_train.py (the definition against independent implementations, no GPU) and tests/test_gpu_train.py
(``train_device`` against ``train_host``, byte for byte): small families, their data, the torch restatement of the graph and the
planted-structure data of the learning test."""
import numpy as np

from sparrowrecsys_amd import trainer as T

F = np.float32


def family(vocabs, kinds, emb_dim, n_dense, widths):
    """A family over tiny vocabularies.  The first Dense kernel's rows: the LAST id column's block, the numerics, then the other
    columns' blocks with their dimensions reversed -- no input row sits where its column and dimension would put it by default."""
    cols = [("c%d" % i, k, int(v)) for i, (v, k) in enumerate(zip(vocabs, kinds))]
    C = len(cols)
    xcol = [C - 1] * emb_dim + [-1] * n_dense
    xsub = list(range(emb_dim)) + list(range(n_dense))
    for c in range(C - 1):
        xcol += [c] * emb_dim
        xsub += list(range(emb_dim))[::-1]
    fam = T.Family(cols, ["emb/c%d" % i for i in range(C)], int(emb_dim), xcol, xsub, int(n_dense), [int(h) for h in widths],
                   ["dense%d" % i for i in range(len(widths))] + ["head"])
    T._check_family(fam)
    return fam


def weights(fam, seed=0, scale=1.0):
    """Glorot-sized kernels, small biases, table rows of unit scale: every ReLU has units on both sides."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shape in T.param_shapes(fam).items():
        if k.startswith("emb/"):
            w[k] = (rng.standard_normal(shape) / np.sqrt(shape[1]) * scale).astype(F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            w[k] = (rng.uniform(-lim, lim, size=shape) * scale).astype(F)
        else:
            w[k] = (rng.uniform(-0.1, 0.1, size=shape) * scale).astype(F)
    return w


def data(fam, n, seed=0, none_rate=0.25):
    """``(ids [n, C] int32, dense [n, F] float32, labels [n] float32)``: ids uniform over the vocabulary, genre columns -1 at
    ``none_rate``, numerics standard normal, labels fair coins."""
    rng = np.random.default_rng(seed + 1000)
    ids = np.stack([rng.integers(0, v, size=n) for _, _, v in fam.columns], axis=1).astype(np.int32)
    for c, (_, k, _) in enumerate(fam.columns):
        if k == "genre":
            ids[rng.random(n) < none_rate, c] = -1
    return ids, rng.standard_normal((n, fam.n_dense)).astype(F), (rng.random(n) < 0.5).astype(F)


def torch_gradients(fam, w, ids, dense, labels, dtype):
    """The same graph in torch on the CPU (``torch.nn.functional``), mean binary cross-entropy through the logit, autograd in
    ``dtype``.  -> ``({name: gradient as float64 numpy}, p)``; a table's gradient is dense, ``[vocab, emb_dim]``."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad=True) for k, v in w.items()}
    ids_t = torch.from_numpy(np.asarray(ids, dtype=np.int64))
    blocks = []
    for c, tab in enumerate(fam.tables):
        ok = (ids_t[:, c] >= 0).to(dtype)[:, None]
        blocks.append(Fn.embedding(ids_t[:, c].clamp(min=0), p[tab]) * ok)
    dn = torch.tensor(np.asarray(dense, dtype=np.float64), dtype=dtype)
    x = torch.stack([dn[:, s] if c < 0 else blocks[c][:, s] for c, s in zip(fam.xcol, fam.xsub)], dim=1)
    for name in fam.layers[:-1]:
        x = Fn.relu(Fn.linear(x, p[name + "/kernel"].t(), p[name + "/bias"]))
    logit = Fn.linear(x, p["head/kernel"].t(), p["head/bias"])[:, 0]
    loss = Fn.binary_cross_entropy_with_logits(logit, torch.tensor(np.asarray(labels, dtype=np.float64), dtype=dtype), reduction="mean")
    loss.backward()
    return {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}, torch.sigmoid(logit).detach().numpy()


# ---- the learning test's data: 50 movies and 200 users with 4-dimensional standard-normal teacher vectors, logit = 1.5 <t_m, t_u>,
# ---- labels Bernoulli of its sigmoid; 16 384 training and 4 096 held-out rows; one seed
PLANTED_SEED, PLANTED_MOVIES, PLANTED_USERS, PLANTED_TRAIN, PLANTED_TEST = 20240, 50, 200, 16384, 4096


def planted():
    """-> ``(train, test, teacher_test)``: ``train`` / ``test`` = ``(ids [n, 2] int32 (movie, user), labels [n] float32)``,
    ``teacher_test`` the teacher's probabilities of the held-out rows."""
    rng = np.random.default_rng(PLANTED_SEED)
    tm, tu = rng.standard_normal((PLANTED_MOVIES, 4)), rng.standard_normal((PLANTED_USERS, 4))
    n = PLANTED_TRAIN + PLANTED_TEST
    mv, us = rng.integers(0, PLANTED_MOVIES, size=n), rng.integers(0, PLANTED_USERS, size=n)
    prob = 1.0 / (1.0 + np.exp(-1.5 * (tm[mv] * tu[us]).sum(axis=1)))
    y = (rng.random(n) < prob).astype(F)
    ids = np.stack([mv, us], axis=1).astype(np.int32)
    k = PLANTED_TRAIN
    return (ids[:k], y[:k]), (ids[k:], y[k:]), prob[k:]


def planted_model(seed=0):
    """NeuralCF at the reference widths over the planted vocabularies, the reference initialisers."""
    from sparrowrecsys_amd import models as M
    mo = M.NeuralCF(seed=seed, movie_buckets=PLANTED_MOVIES, user_buckets=PLANTED_USERS)
    mo.set_weights(mo.init_weights(seed, trained_like=False))
    return mo


def sigmoid_grid():
    """A fixed grid: zero, every float32 exponent from the subnormals to 2^7 at four significands and both signs, the range
    reduction's boundaries (k + 1/2) ln 2 with their neighbours and the multiples of ln 2 for every k in [-126, 126], 7 201 evenly
    spaced points of [-90, 90], and the saturation ends with their neighbours."""
    xs = [0.0] + [s * 2.0 ** e for e in range(-149, 8) for s in (1.0, 1.25, 1.5, 1.9999999)]
    xs = np.array(xs, dtype=F)
    ln2, ks = F(0.6931471805599453), np.arange(-126, 127).astype(F)
    half = ((ks + F(0.5)) * ln2).astype(F)
    bounds = np.concatenate([half, np.nextafter(half, F(np.inf)), np.nextafter(half, F(-np.inf)), (ks * ln2).astype(F)])
    ends = np.array([87.0, -87.0, 88.0, -88.0, 100.0, -100.0, 1e30, -1e30, 3.4e38, -3.4e38, np.nextafter(F(87), F(100)), np.nextafter(F(-87), F(-100))], dtype=F)
    return np.unique(np.concatenate([xs, -xs, bounds, np.linspace(-90, 90, 7201).astype(F), ends]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
