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
and the loss up to the order of a float64 sum; the exact rank statistic (``exact_roc_auc``) needs every score and stays on the host."""
from __future__ import annotations

import numpy as np

EPS = 1e-7


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
    Not provided: the exact rank-statistic AUC (``exact_roc_auc``), which needs every score and stays on the host.

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
