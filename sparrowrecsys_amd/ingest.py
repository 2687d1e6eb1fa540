"""Ingest: CSV text -> the packed ``ids [B,F] int32`` / ``dense [B,N] float32`` arrays in ONE native pass, on the host
(``sprk_pack_csv`` in libsparrow_hip.so, plain C++: no GPU involved) or on the device (``sprk_pack_csv_device``: HIP kernels
over the raw text in HBM, same bits).

The reference reads its sample files with ``tf.data.experimental.make_csv_dataset(..., na_value="0",
ignore_errors=True)`` (DeepFM.py:14-22) and resolves the feature columns inside the graph (DeepFM.py:54-76);
``schema.read_samples_csv`` + ``pack_ids`` + ``pack_dense`` restate that in Python: the definition of the result, and per-element
Python loops for every string column (0.2 - 0.25 M rows/s from object strings).  Same semantics here: empty int -> 0,
empty float -> 0.0, genre string -> vocabulary position or -1, rows of the wrong width dropped, identity ids outside
their bucket range -> ``ValueError``.

A dict of COLUMNS (what ``model.predict(features)`` gets) has the same two native routes: :func:`pack_columns` (host threads,
``sprk_pack_columns``) and :func:`pack_columns_device` (``sprk_pack_columns_device``: k_pack_columns.h).  Both convert the listed
storage kinds with the Python packer's bits or DECLINE the batch (return ``None``); ``CTRModel.pack`` / ``pack_device`` then take the
next route -- device native, host native, Python loop -- so a decline is never an error the caller sees.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .schema import IdColumn, NUMERIC_KEYS


def pack_csv(text, id_columns: Sequence[IdColumn], numeric_keys: Sequence[str] = NUMERIC_KEYS,
             max_rows: int = None, threads: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """``text``: the CSV file's content (bytes or str, header line first) -> ``(ids, dense)``.
    ``threads`` > 1: the body is cut at line boundaries and parsed on that many host threads (``sprk_pack_csv_mt``);
    outputs and the first error are identical for any thread count."""
    if isinstance(text, str):
        text = text.encode("utf-8")
    lib = L.load_library()
    if max_rows is None:
        max_rows = text.count(b"\n") + 1
    n_id, n_dense = len(id_columns), len(numeric_keys)
    cols = (L.CsvCol * max(n_id, 1))()
    for j, c in enumerate(id_columns):
        cols[j].name, cols[j].kind, cols[j].vocab = c.key.encode(), 1 if c.kind == "genre" else 0, c.vocab
    names = (C.c_char_p * max(n_dense, 1))(*[k.encode() for k in numeric_keys])
    ids = np.empty((max_rows, n_id), dtype=np.int32)
    dense = np.empty((max_rows, n_dense), dtype=np.float32)
    rows = C.c_int32(0)
    L.check(lib.sprk_pack_csv_mt(text, C.c_size_t(len(text)), cols, n_id, names, n_dense, max_rows, int(max(1, threads)),
                                 C.c_void_p(ids.ctypes.data), C.c_void_p(dense.ctypes.data), C.byref(rows)))
    return ids[:rows.value], dense[:rows.value]


def pack_csv_file(path: str, id_columns: Sequence[IdColumn], numeric_keys: Sequence[str] = NUMERIC_KEYS,
                  max_rows: int = None, threads: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    with open(path, "rb") as f:
        return pack_csv(f.read(), id_columns, numeric_keys, max_rows, threads)


def pack_csv_device(text, id_columns: Sequence[IdColumn], numeric_keys: Sequence[str] = NUMERIC_KEYS, max_rows: int = None,
                    stream=None):
    """The same packing on the GPU (``sprk_pack_csv_device``: k_csv_pack.h): ``text`` is the CSV content as bytes / str (copied
    to the device once, as raw text) or a ``torch.uint8`` device tensor already holding it; returns DEVICE tensors
    ``(ids [rows, F] int32, dense [rows, N] float32)`` ready for ``Engine.forward``.  Bit-identical to :func:`pack_csv` for the
    values CSV sample files hold (plain decimals of at most 15 digits); quoted fields or other number spellings raise
    (``SparrowHipError``) and name the row -- use :func:`pack_csv` for such files.  There is no silent host fallback."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("pack_csv_device needs a HIP device (use pack_csv for the host tokenizer)")
    if isinstance(text, str):
        text = text.encode("utf-8")
    if isinstance(text, (bytes, bytearray, memoryview)):
        n = len(text)
        if n:
            import warnings
            with warnings.catch_warnings():                       # (a read-only view of the bytes: it is only copied from)
                warnings.simplefilter("ignore")
                host = torch.from_numpy(np.frombuffer(text, dtype=np.uint8))
        else:
            host = torch.empty(0, dtype=torch.uint8)
        buf = torch.empty(n + 16, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))   # (256-byte aligned)
        buf[:n].copy_(host, non_blocking=False)
    else:
        if text.dtype != torch.uint8 or not text.is_cuda or not text.is_contiguous() or text.data_ptr() % 16:
            raise ValueError("pack_csv_device: a contiguous, 16-byte aligned torch.uint8 device tensor is required")
        buf, n = text, text.numel()
    lib = L.load_library()
    if max_rows is None:
        max_rows = int((buf[:n] == 10).sum().item()) + 1 if n else 0
    n_id, n_dense = len(id_columns), len(numeric_keys)
    cols = (L.CsvCol * max(n_id, 1))()
    for j, c in enumerate(id_columns):
        cols[j].name, cols[j].kind, cols[j].vocab = c.key.encode(), 1 if c.kind == "genre" else 0, c.vocab
    names = (C.c_char_p * max(n_dense, 1))(*[k.encode() for k in numeric_keys])
    ids = torch.empty((max(max_rows, 1), n_id), dtype=torch.int32, device=buf.device)
    dense = torch.empty((max(max_rows, 1), n_dense), dtype=torch.float32, device=buf.device)
    rows = C.c_int32(0)
    if stream is None:
        stream = torch.cuda.current_stream(buf.device).cuda_stream
    # the library launches on (and allocates its scratch on) the CURRENT device: make that the text's device
    with torch.cuda.device(buf.device):
        L.check(lib.sprk_pack_csv_device(C.c_void_p(buf.data_ptr()), C.c_size_t(n), cols, n_id, names, n_dense, int(max_rows),
                                         C.c_void_p(ids.data_ptr()), C.c_void_p(dense.data_ptr()), C.byref(rows), C.c_void_p(stream)))
    return ids[:rows.value], dense[:rows.value]


# ---- a dict of columns -> packed ids / dense --------------------------------------------------------------------------------
_tls = threading.local()
_NUMPY_STORAGE = {"b1": L.COL_BOOL, "i1": L.COL_I8, "i2": L.COL_I16, "i4": L.COL_I32, "i8": L.COL_I64, "u1": L.COL_U8, "u2": L.COL_U16,
                  "u4": L.COL_U32, "f4": L.COL_F32, "f8": L.COL_F64}
_TORCH_STORAGE = None


def force_python() -> bool:
    """``SPRK_PACK_NATIVE=0``: ``model.pack`` / ``model.predict`` use the Python packer alone (the route before the native packers
    existed; kept for A/B runs -- scripts/predict_dict_rate.py)."""
    return os.environ.get("SPRK_PACK_NATIVE", "")[:1] == "0"


def default_threads() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(8, n))


def note_route(route: Optional[str]):
    _tls.route = route


def last_pack_route() -> Optional[str]:
    """The route of this thread's last column pack: ``"device"`` / ``"host"`` (the native packers; cross-checked with
    ``sprk_pack_last_route``), ``"python"`` (``model.pack`` / ``pack_device`` fell back to schema.pack_ids / pack_dense), ``None`` = the
    last native call declined (or there was none)."""
    r = getattr(_tls, "route", None)
    if r in ("device", "host"):
        assert int(L.load_library().sprk_pack_last_route()) == (2 if r == "device" else 1)
    return r


def _torch_storage(dtype):
    global _TORCH_STORAGE
    if _TORCH_STORAGE is None:
        import torch
        _TORCH_STORAGE = {torch.bool: L.COL_BOOL, torch.int8: L.COL_I8, torch.int16: L.COL_I16, torch.int32: L.COL_I32, torch.int64: L.COL_I64,
                          torch.uint8: L.COL_U8, torch.float32: L.COL_F32, torch.float64: L.COL_F64}
    return _TORCH_STORAGE.get(dtype)


class _Views:
    """The columns of one batch as ``sprk_pack_col`` descriptors (no per-element Python: a view per column, one ``str.join`` per
    object column); ``ok`` is False when some column is not a storage kind the native packers take."""

    def __init__(self, features: Mapping, id_columns: Sequence[IdColumn], numeric_keys: Sequence[str], allow_device: bool):
        self.ok = False
        self.keep = []                        # whatever the descriptors point into
        self.rows = 0
        self.any_device = False
        n_id, n_dense = len(id_columns), len(numeric_keys)
        want = [(c.key, L.RULE_GENRE if c.kind == "genre" else L.RULE_IDENTITY, c.vocab) for c in id_columns] + \
               [(k, L.RULE_DENSE, 0) for k in numeric_keys]
        for key, _, _ in want:
            if key not in features:
                return                        # (the Python packer raises the KeyError, at the point where it always did)
        B = None
        for v in features.values():
            try:
                B = len(v)
            except TypeError:
                return
            break
        if not B:
            return
        self.rows = B
        self.ids = (L.PackCol * max(n_id, 1))()
        self.dense = (L.PackCol * max(n_dense, 1))()
        text_index = {}                       # id(column object) -> index in the text block
        parts = []
        seen = {}
        for j, (key, rule, vocab) in enumerate(want):
            d = self.ids[j] if j < n_id else self.dense[j - n_id]
            col = features[key]
            got = seen.get(id(col))
            if got is None:
                got = self._describe(col, B, allow_device, text_index, parts)
                if got is None:
                    return
                seen[id(col)] = got
                self.keep.append(col)
            d.data, d.stride, d.storage, d.width, d.on_device = got
            d.rule, d.vocab, d.name = rule, int(vocab), key.encode()
        if parts:
            try:
                self.text = b"".join(p if isinstance(p, bytes) else p.encode("utf-8") for p in parts)
            except UnicodeError:
                return
        else:
            self.text = None
        self.n_id, self.n_dense = n_id, n_dense
        self.ok = True

    def _describe(self, col, B, allow_device, text_index, parts):
        if hasattr(col, "detach"):            # torch tensor
            if col.dim() != 1 or col.shape[0] != B:
                return None
            st = _torch_storage(col.dtype)
            if st is None:
                return None
            if col.is_cuda:
                if not allow_device:
                    return None
                stride = col.stride(0) * col.element_size()
                if not -(1 << 31) <= stride < (1 << 31):
                    return None
                self.any_device = True
                self.device = col.device
                return (col.data_ptr(), stride, st, 0, 1)
            col = col.detach().numpy()
            self.keep.append(col)
        if not isinstance(col, np.ndarray):
            if not isinstance(col, (list, tuple)) or len(col) != B:
                return None
            if isinstance(col[0], (str, bytes)):
                return self._text(col, text_index, parts)
            if col[0] is None:
                return None
            col = np.asarray(col)             # (as schema._as_list reads a list of numbers)
            self.keep.append(col)
        if col.ndim != 1 or col.shape[0] != B:
            return None
        dt = col.dtype
        if dt.kind == "O":
            return self._text(col.tolist(), text_index, parts)
        if not dt.isnative:
            return None
        if dt.kind == "S":
            if not 1 <= dt.itemsize <= 65535:
                return None
            return (col.ctypes.data, col.strides[0], L.COL_BYTES, dt.itemsize, 0)
        if dt.kind == "U":
            if not 1 <= dt.itemsize // 4 <= 65535:
                return None
            return (col.ctypes.data, col.strides[0], L.COL_UCS4, dt.itemsize // 4, 0)
        st = _NUMPY_STORAGE.get(dt.kind + str(dt.itemsize)) if dt.kind in "biuf" else None
        if st is None:                        # uint64, float16, long double, complex, datetimes, ...
            return None
        return (col.ctypes.data, col.strides[0], st, 0, 0)

    def _text(self, values, text_index, parts):
        # one join per column; it raises TypeError by itself when an element is not a str (bytes): the homogeneity check.  A field
        # that holds a newline shifts the count and the native packer declines the block.
        try:
            joined = ("\n" if isinstance(values[0], str) else b"\n").join(values)
        except TypeError:
            return None
        parts.append(joined)
        parts.append("\n" if isinstance(joined, str) else b"\n")
        return (None, 0, L.COL_TEXT, len(parts) // 2 - 1, 0)


def _finish(rc: int, route: str):
    """OK -> True; a decline -> False; the range error -> ValueError with pack_ids' message; anything else raises."""
    if rc == L.EKIND:
        note_route(None)
        return False
    note_route(route)
    L.check(rc)
    return True


def pack_columns(features: Mapping, id_columns: Sequence[IdColumn], numeric_keys: Sequence[str] = NUMERIC_KEYS,
                 threads: Optional[int] = None) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """``{name: column}`` -> HOST arrays ``(ids [B, F] int32, dense [B, N] float32)`` through ``sprk_pack_columns`` (host threads, no
    GPU involved), bit-identical to ``schema.pack_ids`` / ``pack_dense`` -- or ``None`` when the batch is DECLINED (a storage kind or
    a value the native packer does not convert exactly: the caller's next route decides; nothing is raised).  An identity id outside
    its bucket range raises ``pack_ids``' ``ValueError``.  Columns: numpy arrays of native numeric dtypes (any stride), ``S`` / ``U``
    arrays, object arrays / lists of ``str`` (or of ``bytes``), CPU torch tensors."""
    note_route(None)
    v = _Views(features, id_columns, numeric_keys, allow_device=False)
    if not v.ok:
        return None
    lib = L.load_library()
    ids = np.empty((v.rows, v.n_id), dtype=np.int32)
    dense = np.empty((v.rows, v.n_dense), dtype=np.float32)
    rc = lib.sprk_pack_columns(v.ids, v.n_id, v.dense, v.n_dense, v.text, C.c_size_t(len(v.text) if v.text is not None else 0), v.rows,
                               int(threads if threads else default_threads()), C.c_void_p(ids.ctypes.data), C.c_void_p(dense.ctypes.data))
    return (ids, dense) if _finish(rc, "host") else None


def pack_columns_device(features: Mapping, id_columns: Sequence[IdColumn], numeric_keys: Sequence[str] = NUMERIC_KEYS,
                        threads: Optional[int] = None, stream=None, device=None):
    """The same on the GPU (``sprk_pack_columns_device``: k_pack_columns.h) -> DEVICE tensors ``(ids, dense)`` ready for
    ``Engine.forward``, or ``None`` when the batch is declined.  numpy columns are staged by the library (pinned buffer, one
    asynchronous copy); CUDA torch tensors -- also strided views such as ``hist[:, i]`` of a ``[B, T]`` matrix -- are read in place.
    The device twin converts numeric strings of at most 15 significant digits and a decimal exponent within +-22 and declines the
    rest (:func:`pack_columns` converts those).  Synchronises the stream, so a bad id raises here."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("pack_columns_device needs a HIP device (use pack_columns for the host packer)")
    note_route(None)
    v = _Views(features, id_columns, numeric_keys, allow_device=True)
    if not v.ok or v.n_id + v.n_dense > L.PACK_MAX_COLS:
        return None
    if device is None:
        device = v.device if v.any_device else torch.device("cuda", torch.cuda.current_device())
    lib = L.load_library()
    ids = torch.empty((v.rows, v.n_id), dtype=torch.int32, device=device)
    dense = torch.empty((v.rows, v.n_dense), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        rc = lib.sprk_pack_columns_device(v.ids, v.n_id, v.dense, v.n_dense, v.text, C.c_size_t(len(v.text) if v.text is not None else 0),
                                          v.rows, int(threads if threads else default_threads()), C.c_void_p(ids.data_ptr()),
                                          C.c_void_p(dense.data_ptr()), C.c_void_p(stream))
    return (ids, dense) if _finish(rc, "device") else None


def last_device_path() -> int:
    """Which kernels this thread's last ``pack_csv_device`` ran: 1 = the optimistic pass alone (every line a row), 2 = the
    exact keep -> scan -> parse sequence (``sprk_csv_last_path``)."""
    return int(L.load_library().sprk_csv_last_path())


def read_csv_to_device(path: str):
    """The file's bytes as a ``torch.uint8`` device tensor (16 spare bytes behind the text): read straight into pinned host
    memory (one copy out of the page cache) and sent with one asynchronous host -> device copy -- what ``pack_csv_device``
    wants as its input; ``(buffer, n_bytes)``."""
    import os

    import numpy as np
    import torch
    n = os.path.getsize(path)
    host = torch.empty(n + 16, dtype=torch.uint8).pin_memory()
    view = host.numpy()
    with open(path, "rb", buffering=0) as f:
        got = 0
        while got < n:
            k = f.readinto(memoryview(view)[got:n])
            if not k:
                break
            got += k
    if got != n:
        raise IOError("%s: read %d of %d bytes" % (path, got, n))
    view[n:] = 0
    dev = torch.empty(n + 16, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
    dev.copy_(host, non_blocking=True)
    torch.cuda.current_stream().synchronize()                     # the pinned buffer may be released when this returns
    return dev, n
