"""Inputs and restatements shared by tests/test_exact_auc.py and tests/test_gpu_exact_auc.py: Spark's two curves in exact rationals,
written from their description, the defined PR sum in plain Python, and the score sets the tests use."""
import re
from fractions import Fraction

import numpy as np

from sparrowrecsys_amd import metrics as MT
from tests.conftest import ROOT


def kernel_constants():
    """FE_SORT_CAP, FE_SCAN_TILE (k_segments.h: FE_THREADS times 4), EA_PR_RUN and EA_TIE_SCAN_MAX (k_exact_auc.h), read from the sources."""
    seg = open(ROOT + "/sparrowrecsys_amd/csrc/k_segments.h").read()
    ea = open(ROOT + "/sparrowrecsys_amd/csrc/k_exact_auc.h").read()
    threads = int(re.search(r"FE_THREADS = (\d+);", seg).group(1))
    assert re.search(r"FE_SCAN_TILE = 4 \* FE_THREADS;", seg)
    return {"FE_SORT_CAP": int(re.search(r"FE_SORT_CAP = (\d+);", seg).group(1)), "FE_SCAN_TILE": 4 * threads,
            "EA_PR_RUN": int(re.search(r"EA_PR_RUN = (\d+);", ea).group(1)), "EA_TIE_SCAN_MAX": 1 << int(re.search(r"EA_TIE_SCAN_MAX = 1u << (\d+);", ea).group(1))}


def groups_of(labels, scores):
    """Distinct float32 scores (-0.0 as +0.0) in descending order -> (thresholds, pos_g, neg_g) with Python ints."""
    s = np.asarray(scores, dtype=np.float32) + np.float32(0.0)          # (-0.0 + 0.0 = +0.0)
    y = np.asarray(labels) > 0.5
    out = {}
    for v, p in zip(s.tolist(), y.tolist()):
        c = out.setdefault(v, [0, 0])
        c[0 if p else 1] += 1
    th = sorted(out, reverse=True)
    return th, [out[t][0] for t in th], [out[t][1] for t in th]


def spark_areas_exact(labels, scores):
    """(ROC area, PR area) of Spark 2.4's curves as Fractions.  ROC: (0, 0), (fp_g / N, tp_g / P) per threshold, (1, 1); PR:
    (0, prec_1), (tp_g / P, prec_g); trapezoids; a rate over an empty class is 0."""
    _, pos, neg = groups_of(labels, scores)
    P, N = sum(pos), sum(neg)
    tp = fp = 0
    roc = [(Fraction(0), Fraction(0))]
    pr = []
    for p, q in zip(pos, neg):
        tp, fp = tp + p, fp + q
        roc.append((Fraction(fp, N) if N else Fraction(0), Fraction(tp, P) if P else Fraction(0)))
        pr.append((Fraction(tp, P) if P else Fraction(0), Fraction(tp, tp + fp)))
    roc.append((Fraction(1), Fraction(1)))
    pr.insert(0, (Fraction(0), pr[0][1]))
    area = lambda pts: sum((b[0] - a[0]) * (a[1] + b[1]) / 2 for a, b in zip(pts[:-1], pts[1:]))
    return area(roc), area(pr)


def pr_terms(labels, scores):
    """term_g as the definition rounds it, in Python floats (IEEE double, one rounding per operation)."""
    _, pos, neg = groups_of(labels, scores)
    tp = fp = 0
    terms, prev = [], None
    for p, q in zip(pos, neg):
        tp, fp = tp + p, fp + q
        prec = float(tp) / float(tp + fp)
        terms.append(float(p) * (prec + (prec if prev is None else prev)))
        prev = prec
    return terms


def pr_sum_defined(terms, run=None):
    run = MT.PR_RUN if run is None else run
    total = 0.0
    for r in range(0, len(terms), run):
        acc = 0.0
        for t in terms[r:r + run]:
            acc = acc + t
        total = total + acc
    return total


def random_rows(n, seed, grid=None, pos_rate=0.4):
    """n labels (float32 0 / 1, positives likelier at high scores) and float32 scores in (0, 1): continuous, or one of `grid` values."""
    rng = np.random.RandomState(seed)
    p = rng.random_sample(n)
    if grid:
        p = np.floor(p * grid) / grid
    p = p.astype(np.float32)
    y = (rng.random_sample(n) < pos_rate * 0.5 + 0.6 * pos_rate * p.astype(np.float64) * 2).astype(np.float32)
    return y, p


def floats_from_bits(first, count, step=1):
    """count float32 values with consecutive bit patterns first, first + step, ..."""
    return (np.uint32(first) + np.arange(count, dtype=np.uint32) * np.uint32(step)).view(np.float32)


def labels_for(scores, seed):
    return (np.random.RandomState(seed).random_sample(len(scores)) < 0.45).astype(np.float32)


def distinct_groups(G, seed, max_copies=3):
    """Rows with exactly G distinct scores in (0.25, 1), each one to max_copies times, shuffled."""
    rng = np.random.RandomState(seed)
    values = floats_from_bits(0x3e800000 + 16, G, step=1601)               # < 2^23 + 2^24 above 0.25's bits for G <= 8192: below 1.0
    assert G * 1601 < (1 << 24) and len(np.unique(values)) == G
    p = np.repeat(values, rng.randint(1, max_copies + 1, size=G))
    rng.shuffle(p)
    return labels_for(p, seed + 1), p
