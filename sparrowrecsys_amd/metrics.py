"""``model.evaluate``'s numbers (DeepFM.py:117-126: ``loss='binary_crossentropy'``, ``metrics=['accuracy',
tf.keras.metrics.AUC(curve='ROC'), tf.keras.metrics.AUC(curve='PR')]`` -> ``[loss, accuracy, roc_auc, pr_auc]``), computed the
way Keras computes them so that a reference user reads the same figures:

* loss      mean binary cross-entropy with predictions clipped to [1e-7, 1 - 1e-7] (keras/backend.py binary_crossentropy)
* accuracy  ``binary_accuracy``: mean(label == (prediction > 0.5))
* AUC       ``tf.keras.metrics.AUC(num_thresholds=200, summation_method='interpolation')``: confusion counts at 200
            thresholds {-1e-7, 1/199 ... 198/199, 1 + 1e-7} (a prediction is positive when it is GREATER than the threshold);
            ROC: trapezoids over (FPR, TPR); PR: the Davis & Goadrich interpolation of keras/metrics.py ``interpolate_pr_auc``.
            These are approximations of the exact rank statistics by design (the exact ROC-AUC is ``exact_roc_auc``).
Host-side numpy: these functions are the DEFINITION of every number.  ``DeviceMetrics`` keeps the same accumulators in device memory
(``sprk_metrics_update``, csrc/k_metrics.h) and gives these functions' bits for everything that is a count -- accuracy and both AUCs --
and the loss up to the order of a float64 sum.

The exact areas over EVERY distinct score -- what the reference's Spark job reports (offline/spark/evaluate/Evaluator.scala:
``BinaryClassificationMetrics.areaUnderROC()`` / ``areaUnderPR()``) -- are ``exact_auc_host``, the definition, and ``exact_auc_device``,
which gives its bits from scores that lie in device memory (``sprk_exact_auc``, csrc/k_exact_auc.h).  Its ROC
area is the rank statistic ``exact_roc_auc`` computes on the host, which stays as it is."""
from __future__ import annotations

import numpy as np

EPS = 1e-7
PR_RUN = 1024                                                     # groups of one run of the PR sum: part of exact_auc_host's definition
EXACT_AUC_MAX_N = (1 << 31) - 2
EXACT_ERR_SCORE, EXACT_ERR_LABEL = 1, 2


def _confusion(labels: np.ndarray, preds: np.ndarray, num_thresholds: int = 200):
    th = np.array([0.0 - EPS] + [(i + 1) / (num_thresholds - 1) for i in range(num_thresholds - 2)] + [1.0 + EPS])
    y = labels.astype(bool)
    order = np.sort(preds[y]), np.sort(preds[~y])
    # predictions > threshold, per class
    tp = len(order[0]) - np.searchsorted(order[0], th, side="right")
    fp = len(order[1]) - np.searchsorted(order[1], th, side="right")
    fn = len(order[0]) - tp
    tn = len(order[1]) - fp
    return tp.astype(np.float64), fp.astype(np.float64), tn.astype(np.float64), fn.astype(np.float64)


def _div_no_nan(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b != 0, a / np.where(b != 0, b, 1), 0.0)


def auc_from_confusion(tp, fp, tn, fn, curve: str = "ROC") -> float:
    """Keras' AUC from the confusion counts at the thresholds (float64 arrays of one length, as ``_confusion`` and
    ``DeviceMetrics.confusion`` return them): the one expression behind ``keras_auc`` and the device path."""
    n = len(tp)
    if curve == "ROC":
        x = _div_no_nan(fp, fp + tn)
        y = _div_no_nan(tp, tp + fn)
        return float(np.sum((x[:n - 1] - x[1:]) * (y[:n - 1] + y[1:]) / 2.0))
    if curve != "PR":
        raise ValueError("curve must be 'ROC' or 'PR'")
    dtp = tp[:n - 1] - tp[1:]
    p = tp + fp
    dp = p[:n - 1] - p[1:]
    slope = _div_no_nan(dtp, np.maximum(dp, 0))
    intercept = tp[1:] - slope * p[1:]
    ratio = np.where((p[:n - 1] > 0) & (p[1:] > 0), _div_no_nan(p[:n - 1], np.maximum(p[1:], 0)), 1.0)
    inc = _div_no_nan(slope * (dtp + intercept * np.log(ratio)), np.maximum(tp[1:] + fn[1:], 0))
    return float(np.sum(inc))


def keras_auc(labels, preds, curve: str = "ROC", num_thresholds: int = 200) -> float:
    labels, preds = np.asarray(labels).reshape(-1), np.asarray(preds, dtype=np.float64).reshape(-1)
    return auc_from_confusion(*_confusion(labels, preds, num_thresholds), curve)


def exact_roc_auc(labels, preds) -> float:
    """The rank statistic itself (ties count one half) -- what sklearn.metrics.roc_auc_score returns."""
    labels, preds = np.asarray(labels).reshape(-1).astype(bool), np.asarray(preds, dtype=np.float64).reshape(-1)
    order = np.argsort(preds, kind="mergesort")
    ranks = np.empty(len(preds), dtype=np.float64)
    sp = preds[order]
    i = 0
    while i < len(sp):
        j = i
        while j + 1 < len(sp) and sp[j + 1] == sp[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    n_pos, n_neg = int(labels.sum()), int((~labels).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    return float((ranks[labels].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


# ---- the exact areas over every distinct score: Spark's BinaryClassificationMetrics ----------------------------

def exact_auc_error_message(kind: int, row: int) -> str:
    what = {EXACT_ERR_SCORE: "score", EXACT_ERR_LABEL: "label"}.get(int(kind), "input")
    return "exact AUC: the %s of row %d is not finite" % (what, int(row))


class ExactAuc:
    """What ``exact_auc_host`` and ``exact_auc_device`` return.  ``area_under_roc``, ``area_under_pr`` (float), ``n``, ``n_pos``,
    ``n_thresholds`` (the number of distinct scores, G), ``roc_numerator`` (int), ``pr_sum`` (float); with the curve also ``thresholds
    [G] float32`` in descending order and ``tp``, ``fp`` ``[G] uint32``, the positives / negatives with a score >= the threshold
    (``None`` without)."""

    def __init__(self, n, n_pos, n_thresholds, roc_numerator, pr_sum, area_under_roc, area_under_pr, thresholds=None, tp=None, fp=None):
        self.n, self.n_pos, self.n_thresholds, self.roc_numerator = int(n), int(n_pos), int(n_thresholds), int(roc_numerator)
        self.pr_sum, self.area_under_roc, self.area_under_pr = float(pr_sum), float(area_under_roc), float(area_under_pr)
        self.thresholds, self.tp, self.fp = thresholds, tp, fp

    def words(self):
        """The seven words of ``sprk_exact_auc_result``, the doubles as their bits: equal tuples are equal results."""
        bits = lambda v: int(np.float64(v).view(np.uint64))
        return (self.n, self.n_pos, self.n_thresholds, self.roc_numerator, bits(self.pr_sum), bits(self.area_under_roc), bits(self.area_under_pr))

    def _curve(self):
        if self.thresholds is None:
            raise ValueError("the curve was not asked for (return_curve=True)")
        return self.tp.astype(np.float64), self.fp.astype(np.float64)

    def roc_points(self) -> np.ndarray:
        """Spark's ROC curve ``[G + 2, 2]``: (0, 0), (fp_g / N, tp_g / P) per threshold, (1, 1); a rate over an empty class is 0."""
        tp, fp = self._curve()
        P, N = float(self.n_pos), float(self.n - self.n_pos)
        x = fp / N if N else np.zeros_like(fp)
        y = tp / P if P else np.zeros_like(tp)
        return np.concatenate([[[0.0, 0.0]], np.stack([x, y], axis=1), [[1.0, 1.0]]])

    def pr_points(self) -> np.ndarray:
        """Spark 2.4's PR curve ``[G + 1, 2]``: (0, prec_1), then (tp_g / P, prec_g) per threshold; recall over no positive is 0."""
        tp, fp = self._curve()
        P = float(self.n_pos)
        prec = tp / (tp + fp)
        rec = tp / P if P else np.zeros_like(tp)
        return np.concatenate([[[0.0, prec[0]]], np.stack([rec, prec], axis=1)])

    def __repr__(self):
        return "ExactAuc(area_under_roc=%r, area_under_pr=%r, n=%d, n_pos=%d, n_thresholds=%d)" % (self.area_under_roc, self.area_under_pr, self.n, self.n_pos,
                                                                                                   self.n_thresholds)


def _exact_host_labels(labels) -> np.ndarray:
    a = np.asarray(labels).reshape(-1)
    if a.dtype.str[1:] not in ("f4", "i4", "i8", "u1", "b1") or a.dtype.byteorder == ">":      # what DeviceMetrics.update uploads as it is
        with np.errstate(over="ignore", invalid="ignore"):
            a = a.astype(np.float32)
    return a


def exact_score_keys(scores: np.ndarray) -> np.ndarray:
    """The threshold key of finite float32 scores, ``uint32``: ascending keys are descending scores, ``-0.0`` has the key of ``+0.0``."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), u, u ^ np.uint32(0x7fffffff)).astype(np.uint32)
    key[scores == 0] = 0x7fffffff
    return key


def exact_key_scores(keys: np.ndarray) -> np.ndarray:
    k = np.asarray(keys, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k, k ^ np.uint32(0x7fffffff)).astype(np.uint32).view(np.float32)


def exact_auc_host(labels, scores, return_curve: bool = False) -> ExactAuc:
    """The DEFINITION of the exact areas under the ROC and the PR curve (DESIGN.md section 5.15 has the rules and where they come from).

    ``scores``: float32 (anything else is converted), any finite value; a score's threshold is its float32 value, ``-0.0`` taken as
    ``+0.0``.  ``labels``: as ``DeviceMetrics.update`` takes them (float32 / int32 / int64 / uint8 / bool; other dtypes go through
    float32); a sample is positive iff ``label > 0.5``.  Groups ``g = 1 .. G`` are the distinct thresholds in descending order with
    counts ``pos_g``, ``neg_g`` and running sums ``tp_g``, ``fp_g``; ``P = tp_G``, ``N = fp_G``.

    * ``roc_numerator = sum_g neg_g (2 tp_{g-1} + pos_g)``, an integer; ``area_under_roc = float64(roc_numerator) / float64(2 P N)``;
      1.0 when ``N = 0``, else 0.0 when ``P = 0``.
    * ``prec_g = float64(tp_g) / float64(tp_g + fp_g)``, ``prec_0 := prec_1``; ``term_g = float64(pos_g) * (prec_g + prec_{g-1})``, every
      operation rounded on its own.  The terms of ``PR_RUN`` consecutive groups are added in group order from ``+0.0``, the run sums
      in run order from ``+0.0``: that is ``pr_sum``.  ``area_under_pr = pr_sum / float64(2 P)``; 0.0 when ``P = 0``.

    Errors come before anything is computed: the least of ``kind << 32 | row`` over the rows whose score (kind 1) or label (kind 2) is
    not finite raises a ``ValueError`` naming the row; so do ``n = 0`` and ``n > 2^31 - 2``."""
    s = np.asarray(scores)
    if s.dtype != np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            s = s.astype(np.float32)
    s = np.ascontiguousarray(s.reshape(-1))
    lab = _exact_host_labels(labels)
    n = int(s.shape[0])
    if int(lab.shape[0]) != n:
        raise ValueError("exact AUC: %d scores, %d labels" % (n, int(lab.shape[0])))
    if n == 0:
        raise ValueError("exact AUC: no sample")
    if n > EXACT_AUC_MAX_N:
        raise ValueError("exact AUC: at most 2^31 - 2 samples")
    bad = ~np.isfinite(s)
    if bad.any():
        raise ValueError(exact_auc_error_message(EXACT_ERR_SCORE, int(np.flatnonzero(bad)[0])))
    if lab.dtype.kind == "f":
        bad = ~np.isfinite(lab)
        if bad.any():
            raise ValueError(exact_auc_error_message(EXACT_ERR_LABEL, int(np.flatnonzero(bad)[0])))
    positive = lab > 0.5
    keys, inv = np.unique(exact_score_keys(s), return_inverse=True)
    inv = inv.reshape(-1)
    G = len(keys)
    cnt = np.bincount(inv, minlength=G).astype(np.int64)
    pos = np.bincount(inv[positive], minlength=G).astype(np.int64)
    neg = cnt - pos
    tp, fp = np.cumsum(pos), np.cumsum(neg)
    P, N = int(tp[-1]), int(fp[-1])
    numerator = int(np.sum(neg * (2 * (tp - pos) + pos)))                  # <= 2 P N < 2^62: exact in int64
    roc = 1.0 if N == 0 else (0.0 if P == 0 else float(numerator) / float(2 * P * N))
    prec = tp.astype(np.float64) / (tp + fp).astype(np.float64)
    prev = np.concatenate([prec[:1], prec[:-1]])
    term = pos.astype(np.float64) * (prec + prev)
    runs = (G + PR_RUN - 1) // PR_RUN
    padded = np.zeros(runs * PR_RUN, dtype=np.float64)                     # (+0.0 added to a sum that is >= +0.0 changes no bit)
    padded[:G] = term
    run_sum = np.cumsum(padded.reshape(runs, PR_RUN), axis=1)[:, -1]       # cumsum adds one element after the other
    pr_sum = float(np.cumsum(run_sum)[-1])
    pr = 0.0 if P == 0 else pr_sum / float(2 * P)
    out = ExactAuc(n, P, G, numerator, pr_sum, roc, pr)
    if return_curve:
        out.thresholds, out.tp, out.fp = exact_key_scores(keys), tp.astype(np.uint32), fp.astype(np.uint32)
    return out


class _ExactAucCall:
    """An enqueued ``sprk_exact_auc``: ``result()`` is the one synchronisation and the one small copy (the curve, when asked for, is a
    second copy of its ``G`` rows)."""

    def __init__(self, out, curve, keep):
        self._out, self._curve, self._keep = out, curve, keep

    def result(self) -> ExactAuc:
        w = self._out.cpu().numpy()                                        # seven words of result, the error word
        self._keep = None
        err = int(w[7])
        if err != -1:
            raise ValueError(exact_auc_error_message((err >> 32) & 0xffffffff, err & 0xffffffff))
        f = w[4:7].view(np.float64)
        res = ExactAuc(int(w[0]), int(w[1]), int(w[2]), int(w[3:4].view(np.uint64)[0]), float(f[0]), float(f[1]), float(f[2]))
        if self._curve is not None:
            G = res.n_thresholds
            thr, tp, fp = (t[:G].cpu().numpy() for t in self._curve)
            res.thresholds, res.tp, res.fp = thr, tp.view(np.uint32), fp.view(np.uint32)
        return res


def _exact_auc_enqueue(scores, labels, return_curve: bool = False) -> _ExactAucCall:
    import ctypes as C

    import torch

    from . import _lib as L
    who = "exact_auc_device"
    if not torch.cuda.is_available():
        raise RuntimeError("%s: no HIP device is visible (exact_auc_host is the host definition)" % who)
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda or scores.dtype != torch.float32:
        raise ValueError("%s: scores must be a float32 device tensor" % who)
    if scores.dim() == 2 and scores.shape[1] == 1:
        scores = scores[:, 0]
    if scores.dim() != 1:
        raise ValueError("%s: scores must be [n] or [n, 1], not %s" % (who, tuple(scores.shape)))
    n = int(scores.shape[0])
    if n > 1 and scores.stride(0) != 1:
        scores = scores.contiguous()
    dev = scores.device
    if not isinstance(labels, torch.Tensor):
        labels = torch.from_numpy(np.ascontiguousarray(_exact_host_labels(labels))).to(dev, non_blocking=True)
    elif not labels.is_cuda:
        labels = labels.to(dev, non_blocking=True)
    if labels.dim() == 2 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if labels.dim() != 1 or int(labels.shape[0]) != n:
        raise ValueError("%s: %d scores, labels of shape %s" % (who, n, tuple(labels.shape)))
    if labels.device != dev:
        raise ValueError("%s: labels are on %s, the scores on %s" % (who, labels.device, dev))
    storage = DeviceMetrics._storage_of(labels.dtype)
    if storage is None:
        labels, storage = labels.to(torch.float32), L.COL_F32
    if n == 0:
        raise ValueError("exact AUC: no sample")
    if n > EXACT_AUC_MAX_N:
        raise ValueError("exact AUC: at most 2^31 - 2 samples")
    stride = labels.stride(0) if n > 1 else 1
    if stride <= 0:
        labels, stride = labels.contiguous(), 1
    lib = L.load_library()
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        out = torch.zeros(8, dtype=torch.int64, device=dev)
        out[7] = -1                                                        # the error word, ~0
        curve = None
        if return_curve:
            curve = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        ws_bytes = lib.sprk_exact_auc_workspace_bytes(n)
        ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device=dev)    # (torch's allocations are 512-byte aligned)
        null = C.c_void_p(None)
        L.check(lib.sprk_exact_auc(p(scores), p(labels), storage, stride * labels.element_size(), n, p(out),
                                   p(curve[0]) if curve else null, p(curve[1]) if curve else null, p(curve[2]) if curve else null,
                                   C.c_void_p(out.data_ptr() + 56), p(ws), ws.numel() * 8, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return _ExactAucCall(out, curve, (scores, labels, ws))


def exact_auc_device(scores, labels, return_curve: bool = False) -> ExactAuc:
    """``exact_auc_host``'s result, bit for bit, from scores in device memory (``sprk_exact_auc``): ``scores`` a float32 device tensor
    ``[n]`` or ``[n, 1]``, ``labels`` what ``DeviceMetrics.update`` takes -- a device tensor, a strided column view included, or a host
    array, which is uploaded.  Enqueued on the current stream; one synchronisation and one copy of 64 bytes (with ``return_curve`` a
    second copy of the ``G`` curve rows).  Errors are ``exact_auc_host``'s ``ValueError``."""
    return _exact_auc_enqueue(scores, labels, return_curve).result()


def binary_crossentropy(labels, preds) -> float:
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    p = np.clip(np.asarray(preds, dtype=np.float64).reshape(-1), EPS, 1.0 - EPS)
    return float(np.mean(-(y * np.log(p) + (1.0 - y) * np.log(1.0 - p))))


def binary_accuracy(labels, preds, threshold: float = 0.5) -> float:
    y = np.asarray(labels).reshape(-1).astype(np.float64)
    return float(np.mean((np.asarray(preds, dtype=np.float64).reshape(-1) > threshold).astype(np.float64) == y))


def evaluate_scores(labels, preds):
    """``[loss, accuracy, roc_auc, pr_auc]`` -- the list ``model.evaluate`` returns for the reference's compile() call."""
    return [binary_crossentropy(labels, preds), binary_accuracy(labels, preds), keras_auc(labels, preds, "ROC"), keras_auc(labels, preds, "PR")]


class DeviceMetrics:
    """``model.evaluate``'s four numbers as streaming accumulators in DEVICE memory, the way Keras keeps its metrics: counts of
    positives and negatives per threshold bucket, a count of correct predictions, a loss sum, a sample count (a few KB: the layout is
    include/sparrow_hip.h's).  ``update`` folds a batch of device-resident scores in without a score or a label crossing to the host
    and without a synchronisation; ``result`` is the one synchronisation and the one small copy.

    Accuracy and the two AUCs are ``evaluate_scores``' bits (integer counts, then the same expressions); the loss agrees with
    ``binary_crossentropy`` up to the order of the float64 additions and the device's ``log``, and is the same bits on every run.
    Not provided here: the exact areas over every distinct score, which need every score at once -- ``exact_auc_device`` computes them
    from a flat score buffer in device memory.

    One object is not re-entrant: its updates must be ordered on one stream (the current stream of its device).  ``state_dict`` /
    ``merge`` let row-sharded ranks combine their few KB instead of gathering scores; an object that was only merged into needs no GPU."""

    def __init__(self, num_thresholds: int = 200, device=None):
        from . import _lib as L
        if not 2 <= int(num_thresholds) <= L.METRICS_MAX_THRESHOLDS:
            raise ValueError("num_thresholds = %r outside [2, %d]" % (num_thresholds, L.METRICS_MAX_THRESHOLDS))
        self.num_thresholds = int(num_thresholds)
        self.device = device
        self._state = None                                        # the device block: allocated by the first update
        self._merged = self._zero()                               # what merge() added, on the host

    def _zero(self):
        T = self.num_thresholds
        return {"num_thresholds": T, "n": 0, "n_correct": 0, "loss_sum": 0.0, "pos": np.zeros(T + 1, dtype=np.uint64), "neg": np.zeros(T + 1, dtype=np.uint64)}

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._state.device).cuda_stream

    def _device_state(self):
        import ctypes as C

        import torch

        from . import _lib as L
        if self._state is None:
            if not torch.cuda.is_available():
                raise RuntimeError("DeviceMetrics.update: no HIP device is visible (evaluate_scores is the host path)")
            dev = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
            nbytes = L.load_library().sprk_metrics_state_bytes(self.num_thresholds)
            self._state = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            with torch.cuda.device(dev):
                L.check(L.load_library().sprk_metrics_reset(C.c_void_p(self._state.data_ptr()), nbytes, self.num_thresholds, C.c_void_p(self._stream())))
        return self._state

    def reset(self):
        """Zero every accumulator (asynchronous)."""
        import ctypes as C

        import torch

        from . import _lib as L
        self._merged = self._zero()
        if self._state is not None:
            with torch.cuda.device(self._state.device):
                L.check(L.load_library().sprk_metrics_reset(C.c_void_p(self._state.data_ptr()), self._state.numel() * 8, self.num_thresholds,
                                                            C.c_void_p(self._stream())))

    _TORCH_STORAGE = None

    @classmethod
    def _storage_of(cls, dtype):
        import torch

        from . import _lib as L
        if cls._TORCH_STORAGE is None:
            cls._TORCH_STORAGE = {torch.float32: L.COL_F32, torch.int32: L.COL_I32, torch.int64: L.COL_I64, torch.uint8: L.COL_U8, torch.bool: L.COL_BOOL}
        return cls._TORCH_STORAGE.get(dtype)

    def update(self, scores, labels):
        """Fold ``n`` samples in (asynchronous, on the current stream).  ``scores``: a float32 device tensor ``[n]`` or ``[n, 1]``.
        ``labels``: ``[n]`` or ``[n, 1]``, a device tensor of dtype float32 / int32 / int64 / uint8 / bool -- a strided column view is
        read in place -- or a host array, which is uploaded; other dtypes go through float32."""
        import ctypes as C

        import torch

        from . import _lib as L
        if not isinstance(scores, torch.Tensor) or not scores.is_cuda or scores.dtype != torch.float32:
            raise ValueError("DeviceMetrics.update: scores must be a float32 device tensor")
        if scores.dim() == 2 and scores.shape[1] == 1:
            scores = scores[:, 0]
        if scores.dim() != 1:
            raise ValueError("DeviceMetrics.update: scores must be [n] or [n, 1], not %s" % (tuple(scores.shape),))
        n = int(scores.shape[0])
        if n > 1 and scores.stride(0) != 1:
            scores = scores.contiguous()
        state = self._device_state()
        if scores.device != state.device:
            raise ValueError("DeviceMetrics.update: scores are on %s, the state on %s" % (scores.device, state.device))
        if not isinstance(labels, torch.Tensor):
            host = np.asarray(labels)
            host = host.reshape(-1) if host.ndim != 1 else host
            if host.dtype.str[1:] not in ("f4", "i4", "i8", "u1", "b1") or host.dtype.byteorder == ">":
                host = host.astype(np.float32)
            labels = torch.from_numpy(np.ascontiguousarray(host)).to(state.device, non_blocking=True)
        elif not labels.is_cuda:
            labels = labels.to(state.device, non_blocking=True)
        if labels.dim() == 2 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if labels.dim() != 1 or int(labels.shape[0]) != n:
            raise ValueError("DeviceMetrics.update: %d scores, labels of shape %s" % (n, tuple(labels.shape)))
        if labels.device != state.device:
            raise ValueError("DeviceMetrics.update: labels are on %s, the state on %s" % (labels.device, state.device))
        storage = self._storage_of(labels.dtype)
        if storage is None:
            labels = labels.to(torch.float32)
            storage = L.COL_F32
        if n == 0:
            return
        stride = labels.stride(0) if n > 1 else 1
        if stride <= 0:
            labels, stride = labels.contiguous(), 1
        with torch.cuda.device(state.device):
            L.check(L.load_library().sprk_metrics_update(C.c_void_p(state.data_ptr()), state.numel() * 8, C.c_void_p(scores.data_ptr()),
                                                         C.c_void_p(labels.data_ptr()), storage, stride * labels.element_size(), n,
                                                         C.c_void_p(self._stream())))

    def state_dict(self):
        """The accumulators on the host (synchronises; a few KB): ``num_thresholds``, ``n``, ``n_correct``, ``loss_sum``, ``pos`` /
        ``neg`` ``[T + 1] uint64`` -- what ``merge`` takes."""
        T = self.num_thresholds
        sd = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self._merged.items()}
        if self._state is not None:
            w = self._state[:4 + 2 * (T + 1)].cpu().numpy()
            assert int(w[0]) == T
            sd["n"] += int(w[1])
            sd["n_correct"] += int(w[2])
            sd["loss_sum"] += float(w[3:4].view(np.float64)[0])
            sd["pos"] += w[4:4 + T + 1].view(np.uint64)
            sd["neg"] += w[4 + T + 1:4 + 2 * (T + 1)].view(np.uint64)
        return sd

    def thresholds(self) -> np.ndarray:
        """The threshold table the device compares against (``[T] float64``; ``_confusion``'s, bit for bit)."""
        T = self.num_thresholds
        state = self._device_state()
        return state[4 + 2 * (T + 1):4 + 2 * (T + 1) + T].cpu().numpy().view(np.float64).copy()

    def merge(self, other):
        """Add another object's (or ``state_dict``'s) accumulators to this one's, on the host."""
        sd = other.state_dict() if isinstance(other, DeviceMetrics) else other
        if int(sd["num_thresholds"]) != self.num_thresholds:
            raise ValueError("merge: %d thresholds into %d" % (int(sd["num_thresholds"]), self.num_thresholds))
        m = self._merged
        m["n"] += int(sd["n"])
        m["n_correct"] += int(sd["n_correct"])
        m["loss_sum"] += float(sd["loss_sum"])
        m["pos"] = m["pos"] + np.asarray(sd["pos"], dtype=np.uint64)
        m["neg"] = m["neg"] + np.asarray(sd["neg"], dtype=np.uint64)
        return self

    @staticmethod
    def _confusion_of(sd):
        pos, neg = sd["pos"].astype(np.int64), sd["neg"].astype(np.int64)
        T = int(sd["num_thresholds"])
        # predictions > threshold i = the buckets above i
        tp = (pos.sum() - np.cumsum(pos))[:T]
        fp = (neg.sum() - np.cumsum(neg))[:T]
        fn = pos.sum() - tp
        tn = neg.sum() - fp
        return tp.astype(np.float64), fp.astype(np.float64), tn.astype(np.float64), fn.astype(np.float64)

    def confusion(self):
        """``(tp, fp, tn, fn)`` at the thresholds, float64 -- ``_confusion``'s arrays (synchronises)."""
        return self._confusion_of(self.state_dict())

    def result(self):
        """``[loss, accuracy, roc_auc, pr_auc]`` over everything seen so far: the one synchronisation, the one small copy."""
        sd = self.state_dict()
        if sd["n"] == 0:
            raise ValueError("DeviceMetrics.result: no sample was seen")
        conf = self._confusion_of(sd)
        return [sd["loss_sum"] / float(sd["n"]), float(sd["n_correct"]) / float(sd["n"]), auc_from_confusion(*conf, "ROC"), auc_from_confusion(*conf, "PR")]
