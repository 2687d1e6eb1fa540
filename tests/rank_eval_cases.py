"""Inputs and an independent statement of the ranking metrics, shared by tests/test_rank_eval.py and tests/test_gpu_rank_eval.py."""
import math

import numpy as np

from sparrowrecsys_amd import rankeval as RE

TOP_ITEM = 2**31 - 2                     # the greatest item id an int32 column carries


def case(Q=40, Lp=20, n_users=30, n_items=60, per_truth=6, per_seen=10, seed=0, users="random", empty_every=5, negatives=0.1, duplicates=True):
    """Random lists, truth and seen pairs.  Every ``empty_every``-th user has no truth; truth and seen overlap; the rows come shuffled and
    some twice.  ``users``: "random" (some user twice, some never), "identity" (query_user None) or "beyond" (also users past every
    rated one).  -> a dict of rank_eval_host's arguments."""
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, n_items, size=(Q, Lp)).astype(np.int32)
    pred[rng.random((Q, Lp)) < negatives] = -1
    if users == "identity":
        n_users, qu = max(n_users, Q), None
    else:
        top = n_users if users == "random" else n_users + 7
        qu = rng.integers(0, top, size=Q).astype(np.int32)
        if Q > 1:
            qu[-1] = qu[0]                                                   # one user queried twice
        n_users = top
    tu, ti, su, si = [], [], [], []
    for u in range(n_users if users != "beyond" else n_users - 7):
        if per_truth and not (empty_every and u % empty_every == 0):
            items = rng.choice(n_items, size=min(per_truth, n_items), replace=False)
            tu += [u] * len(items); ti += items.tolist()
        if per_seen:
            items = rng.choice(n_items, size=min(per_seen, n_items), replace=False)
            su += [u] * len(items); si += items.tolist()
    def shuffled(a, b):
        a, b = np.array(a, dtype=np.int32), np.array(b, dtype=np.int32)
        if duplicates and len(a):
            again = rng.integers(0, len(a), size=len(a) // 4 + 1)
            a, b = np.concatenate([a, a[again]]), np.concatenate([b, b[again]])
        order = rng.permutation(len(a))
        return a[order], b[order]
    tu, ti = shuffled(tu, ti)
    su, si = shuffled(su, si)
    return dict(pred=pred, query_user=qu, truth_user=tu, truth_item=ti, seen_user=su, seen_item=si, n_users=n_users)


def sets_of(user, item):
    out = {}
    for u, i in zip(np.asarray(user).tolist(), np.asarray(item).tolist()):
        out.setdefault(u, set()).add(i)
    return out


def spark_per_query(pred, query_user, truth_user, truth_item, seen_user, seen_item, ks):
    """Spark's RankingMetrics loops (precisionAt, recallAt, ndcgAt, meanAveragePrecisionAt) transcribed, per query, over Python sets, the
    list first cleared of negative and seen entries; hit rate and reciprocal rank next to them.  -> (per_query, n_relevant, n_ranked)."""
    truth = sets_of(truth_user, truth_item)
    seen = sets_of(seen_user, seen_item) if seen_user is not None else {}
    Q = len(pred)
    per_query, n_relevant, n_ranked = np.zeros((Q, len(ks), 6)), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
    for q in range(Q):
        u = q if query_user is None else int(query_user[q])
        lab = truth.get(u, set())
        p = [int(x) for x in pred[q] if x >= 0 and int(x) not in seen.get(u, set())]
        n_relevant[q], n_ranked[q] = len(lab), len(p)
        if not lab:
            continue                                                       # (Spark logs a warning and returns 0.0)
        for j, k in enumerate(ks):
            cnt = sum(1 for x in p[:k] if x in lab)
            precision, recall = cnt / k, cnt / len(lab)
            n, max_dcg, dcg = min(max(len(p), len(lab)), k), 0.0, 0.0
            for i in range(n):
                gain = 1.0 / math.log(i + 2)
                if i < len(p) and p[i] in lab:
                    dcg += gain
                if i < len(lab):
                    max_dcg += gain
            c, prec_sum = 0, 0.0
            for i in range(min(k, len(p))):
                if p[i] in lab:
                    c += 1
                    prec_sum += c / (i + 1)
            first = next((i for i, x in enumerate(p[:k]) if x in lab), None)
            per_query[q, j] = (precision, recall, dcg / max_dcg, prec_sum / min(len(lab), k), 1.0 if cnt else 0.0, 0.0 if first is None else 1.0 / (first + 1))
    return per_query, n_relevant, n_ranked


def chunked_sums(per_query):
    """The definition's order restated: 256 consecutive queries from +0.0, then the partials from +0.0."""
    Q, n_ks, _ = per_query.shape
    out = np.zeros((n_ks, 6))
    for j in range(n_ks):
        for m in range(6):
            parts = []
            for c in range((Q + 255) // 256):
                s = 0.0
                for q in range(256 * c, min(256 * c + 256, Q)):
                    s += float(per_query[q, j, m])
                parts.append(s)
            t = 0.0
            for s in parts:
                t += s
            out[j, m] = t
    return out


FIELDS = ("per_query", "n_relevant", "n_ranked", "sums", "counts")


def same(got: RE.RankEval, want: RE.RankEval):
    """The five outputs, byte for byte."""
    for name in FIELDS:
        a, b = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name
