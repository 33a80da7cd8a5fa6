"""What the graph-side host modules share (node2vec.py, link_prediction.py, kg_baseline_model.py, transe.py): reading and
numbering names, moving inputs to the device, the two SGD trainers' launch schedule. Functions only; see csrc/graph_common.h."""
import os

import numpy as np

from . import _hip as hip


def read_columns(obj, sep: str, names) -> tuple:
    """One list per column of ``names``: from a TSV path or a DataFrame with those columns, or from ``len(names)``-tuples."""
    import pandas as pd

    if isinstance(obj, (str, os.PathLike)):
        obj = pd.read_csv(obj, sep=sep, usecols=list(names))
    if hasattr(obj, "columns"):
        return tuple(obj[c].tolist() for c in names)
    rows = [tuple(r) for r in obj]
    if any(len(r) != len(names) for r in rows):
        raise ValueError(f"rows of {len(names)} values ({', '.join(names)}) expected")
    return tuple([r[i] for r in rows] for i in range(len(names)))


def factorize_names(*columns):
    """``(codes int [n, k], names)`` of k equally long columns: ONE numbering by first appearance, row by row, column by column."""
    import pandas as pd

    inter = np.empty(len(columns) * len(columns[0]), dtype=object)
    for i, col in enumerate(columns):
        inter[i::len(columns)] = col
    codes, uniques = pd.factorize(inter)          # first-appearance order
    return codes.reshape(-1, len(columns)), list(uniques)


def need_gpu(what: str):
    """torch, or ``StonkHipError(what)`` without a GPU: the kernels have no CPU fallback."""
    import torch

    if not torch.cuda.is_available():
        raise hip.StonkHipError(what)
    return torch


def as_tensor(x, dtype):
    """``x`` itself if it is a tensor (device, dtype and strides are the caller's to check), else a CPU tensor of ``dtype``."""
    import torch

    np_dtype = {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64}[dtype]
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np_dtype))


def to_device(x, dtype, device=None):
    """A tensor or array-like as a contiguous tensor of ``dtype`` on ``device`` (default: the current GPU)."""
    return as_tensor(x, dtype).to(device="cuda" if device is None else device, dtype=dtype).contiguous()


def csr_to_device(rowptr, col, device=None):
    """``(device, rowptr int64, col int32)``; an edgeless graph gets one unused ``col`` entry (the kernels take no null)."""
    import torch

    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    cl = to_device(col, torch.int32, dev) if len(col) else torch.zeros(1, dtype=torch.int32, device=dev)
    return dev, to_device(rowptr, torch.int64, dev), cl


def cuts(n: int, parts: int) -> list:
    """The ``parts + 1`` bounds that cut [0, n) into ``parts`` consecutive ranges whose sizes differ by one at most."""
    return [n * i // parts for i in range(parts + 1)]


def decayed_lr(lr: float, min_lr, i: int, n_launches: int) -> float:
    """The step size of launch i: ``lr`` falling linearly towards ``min_lr`` over the run (constant without one)."""
    return lr if min_lr is None else lr - (lr - min_lr) * i / n_launches


def epoch_means(loss_buffer, epoch_of, epochs: int) -> list:
    """Mean loss per epoch of a [launches, 2] tensor of (loss sum, term count) rows; ``epoch_of[i]``: the epoch of launch i."""
    per, epoch_of = loss_buffer.double().cpu().numpy(), np.asarray(epoch_of)
    return [float(per[epoch_of == e, 0].sum() / max(per[epoch_of == e, 1].sum(), 1.0)) for e in range(epochs)]
