"""Inputs shared by tests/test_item2vec.py, tests/test_gpu_item2vec.py and scripts/item2vec_rate.py: small rating files with the
edges the sequence kernels have (equal timestamps, ratings on both sides of 3.5, rare items, one long user), and the clustered
corpus behind the choice of the trainer's default round (docs/item2vec_results.md)."""
import numpy as np

from sparrowrecsys_amd import item2vec as IV


def ratings(seed=0, n_users=40, n_items=30, n=900, long_user=None, long_len=0, grouped=False):
    """-> dict of columns.  Timestamps are drawn from few values, so ties abound; ratings are half stars, about 60 % of them >= 3.5;
    the items' popularity is skewed, so some fall below min_count.  ``long_user`` gets ``long_len`` more rows; ``grouped`` sorts the
    rows by user (stable), otherwise they are shuffled."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_users, n)
    m = np.minimum((rng.random(n) ** 2 * n_items).astype(np.int64), n_items - 1)
    if long_user is not None:
        u = np.concatenate([u, np.full(long_len, long_user)])
        m = np.concatenate([m, rng.integers(0, n_items, long_len)])
    r = (rng.integers(1, 11, len(u)) * 0.5).astype(np.float32)
    r[rng.random(len(u)) < 0.35] = 4.0
    t = rng.integers(1_000_000, 1_000_000 + max(len(u) // 3, 2), len(u)).astype(np.int64)
    order = np.argsort(u, kind="stable") if grouped else rng.permutation(len(u))
    return {"userId": u[order].astype(np.int64), "movieId": m[order].astype(np.int64), "rating": r[order], "timestamp": t[order]}


def sequences(lengths, n_items, seed=0):
    """Sequences of the given lengths over items [0, n_items), every item often enough to be in the vocabulary when the lengths allow."""
    rng = np.random.default_rng(seed)
    total = int(np.sum(lengths))
    items = np.concatenate([np.arange(n_items)] * (total // max(n_items, 1) + 1))[:total]
    items = rng.permutation(items).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return off, items


CLUSTER_ITEMS, CLUSTERS, CLUSTER_SENTENCES, CLUSTER_LENGTH = 200, 10, 410, 20


def clustered_corpus(seed=0):
    """200 items in 10 clusters of 20; 410 sentences of 20 words, each from one cluster with one word in ten from anywhere: 8 200 words,
    two rounds of 4 096 and a rest.  -> (seq_offsets, seq_items, cluster of every item)."""
    rng = np.random.default_rng(seed)
    per = CLUSTER_ITEMS // CLUSTERS
    cluster = np.arange(CLUSTER_ITEMS) // per
    rows = []
    for s in range(CLUSTER_SENTENCES):
        c = s % CLUSTERS
        w = c * per + rng.integers(0, per, CLUSTER_LENGTH)
        noise = rng.random(CLUSTER_LENGTH) < 0.1
        w[noise] = rng.integers(0, CLUSTER_ITEMS, int(noise.sum()))
        rows.append(w)
    items = np.concatenate(rows).astype(np.int32)
    off = (np.arange(CLUSTER_SENTENCES + 1) * CLUSTER_LENGTH).astype(np.int32)
    return off, items, cluster


def purity(vectors, ids, cluster, k=10):
    """The share of same-cluster items among the ``k`` cosine-nearest neighbours, averaged over the items."""
    v = np.asarray(vectors, dtype=np.float64)
    v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)
    sim = v @ v.T
    np.fill_diagonal(sim, -np.inf)
    near = np.argsort(-sim, axis=1, kind="stable")[:, :k]
    c = np.asarray(cluster)[np.asarray(ids)]
    return float((c[near] == c[:, None]).mean())


def clustered_fit(round, row_cap=32, seed=0, iters=10):
    """:func:`skipgram_host` on the clustered corpus with the defaults of ``item2vec.fit``.  -> (loss, purity, max |syn1|)."""
    off, items, cluster = clustered_corpus()
    vocab = IV.vocabulary_host(np.bincount(items, minlength=CLUSTER_ITEMS), 5)
    corpus = IV.corpus_host(off, items, vocab, CLUSTER_ITEMS)
    out = IV.skipgram_host(corpus, vocab, D=10, window=5, iters=iters, lr=0.025, round=round, row_cap=row_cap, seed=seed)
    return out.loss, purity(out.vectors, vocab.ids, cluster), float(np.abs(out.syn1).max())
