"""Shared cases of tests/test_train_fm.py (the DeepFM_v2 trainer's definition against independent implementations, no GPU) and
tests/test_gpu_train_fm.py (``trainer_fm.train_device`` against ``train_host``, byte for byte): small ``DeepFMv2`` models, weights,
data, the torch restatement of the graph and the planted-structure data of the learning test."""
import numpy as np

from sparrowrecsys_amd import models as M
from sparrowrecsys_amd import trainer_fm as TF
from tests import train_cases as TC

F = np.float32
same_bits = TC.same_bits

REFERENCE_SHAPE = dict(vocabs=(30, 40, 19, 19), kinds=("id", "id", "genre", "genre"), order=(3, 0, 2, 1), emb_dim=10, proj_dim=64, hidden=(32, 16))
ODD_SHAPE = dict(vocabs=(7, 5, 9, 6), kinds=("id", "genre", "id", "genre"), order=(2, 0, 3), emb_dim=3, proj_dim=5, hidden=(17, 1))


def model(vocabs=(6, 5, 9), kinds=("id", "genre", "id"), order=None, emb_dim=3, proj_dim=5, hidden=(5,), seed=0):
    """A ``DeepFMv2`` over tiny vocabularies.  The field keys are chosen so that their name order (= the order of their blocks in
    ``fo_cat/kernel``) is the REVERSE of the field order; ``order`` lists field indices (default: all, reversed)."""
    n = len(vocabs)
    fields = [("f%d" % (n - 1 - i), k, int(v)) for i, (v, k) in enumerate(zip(vocabs, kinds))]
    order = list(range(n))[::-1] if order is None else list(order)
    return M.DeepFMv2(seed=seed, emb_dim=emb_dim, fields=fields, order=[fields[i][0] for i in order], proj_dim=proj_dim, hidden=hidden)


def family(**kw):
    return TF.family_of(model(**kw))


def weights(fam, seed=0, scale=1.0):
    """Glorot-sized kernels, small biases, table rows of unit scale, first-order rows of scale 0.3."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shape in TF.param_shapes(fam).items():
        if k.startswith("emb/"):
            w[k] = (rng.standard_normal(shape) / np.sqrt(shape[1]) * scale).astype(F)
        elif k == "fo_cat/kernel":
            w[k] = (rng.standard_normal(shape) * 0.3 * scale).astype(F)
        elif k.endswith("/kernel"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            w[k] = (rng.uniform(-lim, lim, size=shape) * scale).astype(F)
        else:
            w[k] = (rng.uniform(-0.1, 0.1, size=shape) * scale).astype(F)
    return w


def data(fam, n, seed=0, none_rate=0.25):
    """``train_cases.data``: ids uniform, genre fields -1 at ``none_rate``, numerics standard normal, labels fair coins."""
    return TC.data(fam, n, seed, none_rate)


def small(n, seed=0, **kw):
    fam = family(**kw)
    return (fam, weights(fam, seed)) + data(fam, n, seed)


def torch_logit(fam, p, ids_t, dn, dtype):
    """The graph in torch (``torch.nn.functional``) from a dict of tensors ``p``: -> the logit ``[n]``."""
    import torch
    import torch.nn.functional as Fn
    col = {k: c for c, (k, _, _) in enumerate(fam.fields)}
    first = torch.zeros(ids_t.shape[0], dtype=dtype)
    for c in range(len(fam.fields)):
        ok = (ids_t[:, c] >= 0).to(dtype)
        first = first + Fn.embedding(ids_t[:, c].clamp(min=0) + fam.fo_off[c], p["fo_cat/kernel"])[:, 0] * ok
    first = first + p["fo_cat/bias"][0] + Fn.linear(dn, p["fo_num/kernel"].t(), p["fo_num/bias"])[:, 0]
    vs = []
    for k in fam.order:
        ok = (ids_t[:, col[k]] >= 0).to(dtype)[:, None]
        e = Fn.embedding(ids_t[:, col[k]].clamp(min=0), p["emb/" + k]) * ok
        vs.append(Fn.linear(e, p["proj/%s/kernel" % k].t(), p["proj/%s/bias" % k]))
    vs.append(Fn.linear(dn, p["proj/num/kernel"].t(), p["proj/num/bias"]))
    stack = torch.stack(vs, dim=1)
    s = stack.sum(dim=1)
    fm = s * s - (stack * stack).sum(dim=1)
    x = stack.reshape(stack.shape[0], -1)
    for i in range(len(fam.hidden)):
        x = Fn.relu(Fn.linear(x, p["deep%d/kernel" % i].t(), p["deep%d/bias" % i]))
    cat = torch.cat([first[:, None], fm, x], dim=1)
    return Fn.linear(cat, p["head/kernel"].t(), p["head/bias"])[:, 0]


def torch_gradients(fam, w, ids, dense, labels, dtype):
    """Mean binary cross-entropy through the logit, autograd in ``dtype`` on the CPU.  -> ``({name: gradient as float64 numpy}, p)``."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad=True) for k, v in w.items()}
    logit = torch_logit(fam, p, torch.from_numpy(np.asarray(ids, dtype=np.int64)), torch.tensor(np.asarray(dense, dtype=np.float64), dtype=dtype), dtype)
    loss = Fn.binary_cross_entropy_with_logits(logit, torch.tensor(np.asarray(labels, dtype=np.float64), dtype=dtype), reduction="mean")
    loss.backward()
    return {k: (v.grad.detach().numpy().astype(np.float64) if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}, torch.sigmoid(logit).detach().numpy()


# ---- the learning test: train_cases.planted()'s movies, users and labels; the seven numerics are standard-normal noise of a fixed seed
PLANTED_NOISE_SEED = 515


def planted():
    """-> ``(train, test)``, each ``(ids [n, 2] int32 (movie, user), dense [n, 7] float32, labels [n] float32)``."""
    (ids, y), (tids, ty), _ = TC.planted()
    rng = np.random.default_rng(PLANTED_NOISE_SEED)
    return (ids, rng.standard_normal((len(y), 7)).astype(F), y), (tids, rng.standard_normal((len(ty), 7)).astype(F), ty)


def planted_model(seed=0):
    """DeepFM_v2 at the reference widths (emb_dim 10, proj_dim 64, hidden (32, 16)) over the planted vocabularies, the reference initialisers."""
    mo = M.DeepFMv2(seed=seed, fields=[("movieId", "id", TC.PLANTED_MOVIES), ("userId", "id", TC.PLANTED_USERS)], order=["movieId", "userId"])
    mo.set_weights(mo.init_weights(seed, trained_like=False))
    return mo
