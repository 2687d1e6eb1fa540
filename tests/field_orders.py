"""Field orders the DeepFM plan matchers must follow (tests/test_field_orders_cpu.py, tests/test_gpu_field_orders.py).

The engine re-derives at finalize which field feeds which kernel slot (match_v2_chain, setup_v2_joint, setup_rows_v2 for DeepFM_v2;
setup_deepfm_pairs for the pair-dot DeepFM), each from the plan's segments.  The shapes below give those matchers permutations
that are not the identity, and the weight transforms build the same mathematical model in another way: a kernel slot that reads
the wrong field's weights moves the score, a correct one does not."""
import numpy as np

from sparrowrecsys_amd import models as M

TIGHT = 3e-5                       # tests/test_gpu_parity.py: fp32-class against the fp64 oracle
BATCHES = (4099, 17, 1)

# ---- DeepFM_v2 ------------------------------------------------------------------------------------------------------------------
GENRES3 = [("userGenre1", "genre", 19), ("userGenre2", "genre", 19), ("movieGenre1", "genre", 19)]
# S1: three ids fields of one vocabulary + three genre fields (emb 16, proj 16, deep 32-16: the folded kernels)
S1_FIELDS = [("movieId", "id", 3000), ("userId", "id", 3000), ("userRatedMovie1", "id", 3000)] + GENRES3
# S2: the same with mixed vocabularies
S2_FIELDS = [("movieId", "id", 3000), ("userId", "id", 9000), ("userRatedMovie1", "id", 5000)] + GENRES3
KEYS = [k for k, _, _ in S1_FIELDS]
S1_ORDERS = {
    "identity": list(KEYS),
    "ids-3cycle": ["userId", "userRatedMovie1", "movieId"] + KEYS[3:],
    "reversed": KEYS[::-1],
}
S2_ORDERS = {"6cycle": KEYS[1:] + KEYS[:1]}
# S3 / S4: the reference's four fields in DeepFM_v2.py's own order
REF_FIELDS = M._default_fields()
REF_ORDER = list(M.DeepFMv2.DEFAULT_ORDER)
# S4 at projection 32: two big fields of different vocabularies + two genre fields, the big ones and the genres each swapped
S4_FIELDS = [("movieId", "id", 3000), ("userId", "id", 9000), ("userGenre1", "genre", 19), ("movieGenre1", "genre", 19)]
S4_ORDER = ["userId", "movieGenre1", "movieId", "userGenre1"]

# name -> (fields, order, emb_dim, proj_dim, weight seed): seeds whose output layer does not all but mute the first-order term
V2_CASES = {
    **{"S1-" + k: (S1_FIELDS, o, 16, 16, 33) for k, o in S1_ORDERS.items()},
    **{"S2-" + k: (S2_FIELDS, o, 16, 16, 33) for k, o in S2_ORDERS.items()},
    "S3-reference-order": (REF_FIELDS, REF_ORDER, 16, 16, 33),
    "S4-proj32": (S4_FIELDS, S4_ORDER, 16, 32, 34),
    "S4-reference": (REF_FIELDS, REF_ORDER, 10, 64, 33),
}


def perm_of(fields, order):
    """sigma[g] = index in ``fields`` of embedding group g (the field at position g of ``order``)."""
    names = [k for k, _, _ in fields]
    return [names.index(k) for k in order]


def is_identity(p):
    return all(i == j for i, j in enumerate(p))


def is_involution(p):
    return all(p[p[i]] == i for i in range(len(p)))


def shuffled(fields, seed):
    return [fields[i] for i in np.random.default_rng(seed).permutation(len(fields))]


def v2_identity_order(fields, order, w, proj_dim):
    """The same DeepFM_v2 with ``order`` = the field list: deep0/kernel's proj_dim-row blocks follow the groups (the FM sum of
    squares is symmetric over groups, every other weight is keyed by name).  -> (order, weights)."""
    new_order = [k for k, _, _ in fields]
    k0 = w["deep0/kernel"]
    blocks = [k0[order.index(k) * proj_dim:(order.index(k) + 1) * proj_dim] for k in new_order]
    blocks.append(k0[len(order) * proj_dim:])                     # the numerics' projection stays last
    out = dict(w)
    out["deep0/kernel"] = np.ascontiguousarray(np.concatenate(blocks, axis=0))
    return new_order, out


def swap_fo_blocks(fields, w, a, b, kernel="fo_cat/kernel"):
    """Sensitivity guard: the first-order weights of fields ``a`` and ``b`` exchanged (the first min(vocab) rows of each block)."""
    fo = M.first_order_offsets(fields)
    voc = {k: v for k, _, v in fields}
    n = min(voc[a], voc[b])
    k = w[kernel].copy()
    ra, rb = slice(fo[a], fo[a] + n), slice(fo[b], fo[b] + n)
    k[ra], k[rb] = w[kernel][rb], w[kernel][ra]
    out = dict(w)
    out[kernel] = k
    return out


def guard_pair(fields, order):
    """Two fields ``order`` moves, the pair with the most first-order rows in common (the swap of swap_fo_blocks)."""
    voc = {k: v for k, _, v in fields}
    sig = perm_of(fields, order)
    moved = [order[g] for g in range(len(sig)) if sig[g] != g]
    pairs = [(a, b) for i, a in enumerate(moved) for b in moved[i + 1:]]
    return max(pairs, key=lambda ab: min(voc[ab[0]], voc[ab[1]]))


def v2_w1_applied_twice(fields, order, w):
    """What the fallback of an unfolded DeepFM_v2 read before its fix (match_v2_chain rewrote V2Args::w1 into group order and
    setup_rows_v2 looked it up by first-order position once more): field f scored with the first-order weights of field
    sigma(f).  Only defined for equal vocabularies (otherwise the read leaves the smaller block)."""
    fo = M.first_order_offsets(fields)
    voc = {k: v for k, _, v in fields}
    names = [k for k, _, _ in fields]
    sig = perm_of(fields, order)
    k = w["fo_cat/kernel"].copy()
    for f, key in enumerate(names):
        src = names[sig[f]]
        assert voc[src] == voc[key]
        k[fo[key]:fo[key] + voc[key]] = w["fo_cat/kernel"][fo[src]:fo[src] + voc[src]]
    out = dict(w)
    out["fo_cat/kernel"] = k
    return out


# ---- pair-dot DeepFM --------------------------------------------------------------------------------------------------------------
PAIR_FIELDS_6 = [("movieId", "id", 3000), ("userId", "id", 5000), ("userRatedMovie1", "id", 3000), ("userGenre1", "genre", 19),
                 ("userGenre2", "genre", 19), ("movieGenre1", "genre", 19)]
PAIR_SHAPES = {                    # name -> (fields, pairs, emb_dim)
    "nf4-emb10": (REF_FIELDS, list(M.DeepFM.DEFAULT_PAIRS), 10),
    "nf4-emb16": (REF_FIELDS, list(M.DeepFM.DEFAULT_PAIRS), 16),
    "nf6-emb16": (PAIR_FIELDS_6, [(a, b) for a in ("movieId", "movieGenre1") for b in ("userId", "userRatedMovie1", "userGenre1", "userGenre2")], 16),
}


def _head_rows(fields, pairs):
    n_fo = M.first_order_offsets(fields)["__total__"]
    return n_fo, n_fo + len(pairs)


def pairs_reordered(fields, pairs, w, seed):
    """The pair list in another order, head/kernel's pair rows permuted to match."""
    perm = np.random.default_rng(seed).permutation(len(pairs))
    lo, hi = _head_rows(fields, pairs)
    hk = w["head/kernel"].copy()
    hk[lo:hi] = w["head/kernel"][lo:hi][perm]
    out = dict(w)
    out["head/kernel"] = hk
    return [pairs[i] for i in perm], out


def pairs_flipped(pairs):
    """Every pair's orientation reversed: a dot product, the same model with the same weights."""
    return [(b, a) for a, b in pairs]


def pair_duplicated(fields, pairs, w, i, split=0.25):
    """Pair ``i`` listed twice (appended at the end), its head weight split ``split`` / ``1 - split`` between the two rows."""
    lo, hi = _head_rows(fields, pairs)
    hk = w["head/kernel"]
    row = hk[lo + i].copy()
    new = np.concatenate([hk[:lo + i], row[None] * split, hk[lo + i + 1:hi], row[None] * (1 - split), hk[hi:]], axis=0)
    out = dict(w)
    out["head/kernel"] = np.ascontiguousarray(new, dtype=np.float32)
    return pairs + [pairs[i]], out


def pair_constructions(fields, pairs, w, deep_emb=("movieId", "userId")):
    """-> {name: (fields, pairs, deep_emb, weights)}: the pair-dot model of (fields, pairs, deep_emb, w), built in other ways."""
    deep_emb = list(deep_emb)
    rp, rw = pairs_reordered(fields, pairs, w, seed=len(pairs))
    dp, dw = pair_duplicated(fields, pairs, w, 1)
    both_p, both_w = pairs_reordered(fields, pairs_flipped(pairs), w, seed=3)
    return {
        "fields-shuffled": (shuffled(fields, 11), pairs, deep_emb, w),
        "pairs-reordered": (fields, rp, deep_emb, rw),
        "pairs-flipped": (fields, pairs_flipped(pairs), deep_emb, w),
        "deep-emb-reversed": (fields, pairs, deep_emb[::-1], w),
        "pair-duplicated": (fields, dp, deep_emb, dw),
        "all-at-once": (shuffled(fields, 12), both_p, deep_emb[::-1], both_w),
    }
