"""Graph definitions: ``GraphDefinition`` / ``KNNGraph`` / ``KNNEdges`` / ``MinkowskiKNNEdges`` / ``RadialEdges`` /
``NodesAsPulses`` / ``PercentileClusters`` / ``NodeAsDOMTimeSeries`` / ``IceMixNodes``.

Host-side mirror of ``models/graphs/graph_definition.py:148-248``, ``graphs/graphs.py:13-58``,
``graphs/edges/edges.py:47-117``, ``graphs/edges/minkowski.py:37-99`` and ``graphs/nodes/nodes.py:22-453``.

Difference by design: the reference builds k-NN edges on the CPU, one event
at a time, inside DataLoader workers.  Here a CPU ``Data`` leaves ``edge_index`` unset and the
backbone builds the whole batch's layer-1 graph with one ``gn_knn_graph`` launch on the GPU
(same columns, same k, same result).  On a GPU tensor ``KNNEdges`` runs the HIP kernel at once.
There is no CPU k-NN in this package.
"""
from __future__ import annotations

import os
import warnings
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from numpy.random import Generator, default_rng

from .data import Data
from .detector import Detector
from .model import Model


class NodeDefinition(Model):
    """Pulses -> nodes (``nodes/nodes.py:22-120``).  A subclass names its output columns in
    ``_define_output_feature_names`` and builds the node matrix in ``_construct_nodes``."""

    def __init__(self, input_feature_names: Optional[List[str]] = None) -> None:
        super().__init__()
        if input_feature_names is not None:
            self.set_output_feature_names(input_feature_names)

    def forward(self, x: torch.Tensor):
        graph = self._construct_nodes(x)
        return graph, self._output_feature_names         # AttributeError while the names are not set

    def set_number_of_inputs(self, input_feature_names: List[str]) -> None:
        assert isinstance(input_feature_names, list)
        self.nb_inputs = len(input_feature_names)

    def set_output_feature_names(self, input_feature_names: List[str]) -> None:
        self._output_feature_names = self._define_output_feature_names(list(input_feature_names))

    def _define_output_feature_names(self, input_feature_names: List[str]) -> List[str]:
        raise NotImplementedError

    def _construct_nodes(self, x: torch.Tensor) -> Data:
        raise NotImplementedError

    @property
    def nb_outputs(self) -> int:
        return len(self._output_feature_names)


class NodesAsPulses(NodeDefinition):
    """Each pulse is a node (``nodes/nodes.py:123-132``)."""

    def _define_output_feature_names(self, input_feature_names: List[str]) -> List[str]:
        return input_feature_names

    def _construct_nodes(self, x: torch.Tensor) -> Data:
        return Data(x=x)


def _order_keys(v: np.ndarray, cluster: bool) -> np.ndarray:
    """fp32 values -> uint32 keys that ascend with the values: every NaN one key after +inf; for a cluster column
    ``-0.0`` is taken as ``+0.0``."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    b = v.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    if cluster:
        k[v == 0] = np.uint32(0x80000000)
    k[np.isnan(v)] = np.uint32(0xFFFFFFFF)
    return k


def percentile_clusters_host(x: np.ndarray, cluster_cols: List[int], summ_cols: List[int], percentiles: List[float],
                             add_counts: bool = True) -> np.ndarray:
    """The contract of ``gn_percentile_clusters`` (``include/graphnet_amd.h``) for ONE event in vectorised numpy: fp32
    ``[n, F]`` -> fp32 ``[M, C + S*P + add_counts]``.  Bit for bit what the kernels write, but for the counts column,
    which is numpy's ``log10`` here."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, C, S, P = len(x), len(cluster_cols), len(summ_cols), len(percentiles)
    W = C + S * P + (1 if add_counts else 0)
    if n == 0:
        return np.zeros((0, W), dtype=np.float32)
    keys = [_order_keys(x[:, c], True) for c in cluster_cols]
    order = np.lexsort(tuple(keys))                          # stable; the LAST cluster column is the most significant
    sorted_keys = np.stack([k[order] for k in keys], axis=1)
    head = np.ones(n, dtype=bool)
    head[1:] = (sorted_keys[1:] != sorted_keys[:-1]).any(axis=1)
    start = np.flatnonzero(head)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.cumsum(head) - 1
    M = len(start)
    out = np.empty((M, W), dtype=np.float32)
    out[:, :C] = x[order[start]][:, cluster_cols]            # a cluster's lowest-index pulse comes first in a stable sort
    q = np.asarray(percentiles, dtype=np.float64) / 100
    with np.errstate(invalid="ignore"):
        for s, f in enumerate(summ_cols):
            by_value = np.lexsort((_order_keys(x[:, f], False), rank))      # NaN last inside its cluster
            vals = x[by_value, f].astype(np.float64)
            m = np.add.reduceat((~np.isnan(vals)).astype(np.int64), start)
            h = (m - 1)[:, None] * q[None, :]
            fl = np.floor(h)
            lo = np.maximum(fl.astype(np.int64), 0)
            hi = np.maximum(np.minimum(lo + 1, (m - 1)[:, None]), 0)
            g = h - fl
            a, b = vals[start[:, None] + lo], vals[start[:, None] + hi]
            d = b - a
            r = np.where(g >= 0.5, b - d * (1 - g), a + d * g)
            r[m == 0] = np.nan
            out[:, C + s * P:C + (s + 1) * P] = r.astype(np.float32)
    if add_counts:
        out[:, -1] = np.log10(np.diff(np.append(start, n)).astype(np.float64)).astype(np.float32)
    return out


class PercentileClusters(NodeDefinition):
    """One node per cluster of pulses with equal ``cluster_on`` features - with the DOM position, one node per DOM - and
    every other feature summarised by ``percentiles`` (``nodes/nodes.py:135-217``; argument names, order and defaults
    are the reference's).  Output columns: ``cluster_on + [f"{feature}_pct{p}" ...] + ["counts"]``; ``counts`` is
    ``log10`` of the number of pulses of the cluster.

    The arithmetic is defined operation by operation in ``include/graphnet_amd.h`` (``gn_percentile_clusters``): nodes
    ascend in ``np.lexsort`` order of the cluster columns, percentiles are numpy's method "linear" over the cluster's
    non-NaN values in fp64.  A device tensor takes one ``gn_percentile_clusters`` call; a CPU tensor takes
    :func:`percentile_clusters_host`, the same contract in numpy (the loader path of the reference).  On the device a
    whole batch is clustered by one call: ``GraphDefinition.batch_from_raw``.

    Two definitions where the reference has none or differs:

    * **NaN in a cluster column.**  All NaNs of a column are one value that sorts after ``+inf`` (the reference's
      ``lexsort`` and ``unique`` disagree with each other there); ``-0.0`` clusters with ``+0.0``, as ``np.unique`` has it.
    * **fp32.**  The node matrix is fp32 wherever it is built.  The reference's stand-alone call returns numpy's fp64
      array, which ``GraphDefinition`` casts to ``dtype`` a line later.
    """

    def __init__(self, cluster_on: List[str], percentiles: List[int], add_counts: bool = True,
                 input_feature_names: Optional[List[str]] = None) -> None:
        self._cluster_on = list(cluster_on)
        self._percentiles = list(percentiles)
        self._add_counts = add_counts
        super().__init__(input_feature_names=input_feature_names)

    def _define_output_feature_names(self, input_feature_names: List[str]) -> List[str]:
        summarised = [f for f in input_feature_names if f not in self._cluster_on]
        self._cluster_indices = [input_feature_names.index(f) for f in self._cluster_on]
        self._summarization_indices = [input_feature_names.index(f) for f in summarised]
        names = list(self._cluster_on) + [f"{f}_pct{p}" for f in summarised for p in self._percentiles]
        return names + ["counts"] if self._add_counts else names

    def _indices(self) -> Tuple[List[int], List[int]]:
        if not hasattr(self, "_summarization_indices"):
            raise AttributeError(f"{self.__class__.__name__} was instantiated without `input_feature_names` and they "
                                 "were not set before this call; outside a GraphDefinition pass `input_feature_names`")
        return self._cluster_indices, self._summarization_indices

    def cluster_batch(self, x: torch.Tensor, ptr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(nodes fp32 [M, W], node_ptr int32 [B + 1])`` of the events ``ptr`` marks in ``x``: one device call, or
        the host path event by event for a CPU tensor."""
        cl, sm = self._indices()
        if x.is_cuda:
            from . import ops
            return ops.percentile_clusters(x.to(torch.float32), ptr.to(torch.int32), cl, sm, self._percentiles,
                                           self._add_counts)
        xn, bounds = x.detach().to(torch.float32).numpy(), ptr.tolist()
        parts = [percentile_clusters_host(xn[lo:hi], cl, sm, self._percentiles, self._add_counts)
                 for lo, hi in zip(bounds[:-1], bounds[1:])]
        node_ptr = np.zeros(len(bounds), dtype=np.int32)
        node_ptr[1:] = np.cumsum([len(p) for p in parts])
        nodes = np.concatenate(parts, axis=0) if parts else np.zeros((0, self.nb_outputs), dtype=np.float32)
        return torch.from_numpy(nodes), torch.from_numpy(node_ptr)

    def _construct_nodes(self, x: torch.Tensor) -> Data:
        ptr = torch.tensor([0, int(x.shape[0])], dtype=torch.int32, device=x.device)
        return Data(x=self.cluster_batch(x, ptr)[0])


def dom_time_series_host(x: np.ndarray, id_cols: List[int], time_col: int, charge_col: int = -1) -> np.ndarray:
    """The contract of ``gn_dom_time_series`` (``include/graphnet_amd.h``) for ONE event in vectorised numpy: fp32
    ``[n, F]`` -> fp32 ``[n, F + (charge_col < 0) + 1]``.  Bit for bit what the kernel writes, but for the charge column,
    which is numpy's fp64 ``power`` here."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, F = x.shape
    W = F + (1 if charge_col < 0 else 0) + 1
    out = np.empty((n, W), dtype=np.float32)
    if n == 0:
        return out
    keys = [_order_keys(x[:, time_col], True)] + [_order_keys(x[:, c], True) for c in id_cols]
    order = np.lexsort(tuple(keys))                          # stable; the LAST id column most significant, time least
    t = x[:, time_col]
    if np.isnan(t).any():
        tmin = np.float32(np.nan)
    else:
        tmin = t.min()
        if tmin == 0 and np.signbit(t[t == 0]).any():        # -0.0 before +0.0
            tmin = np.float32(-0.0)
    out[:, :F] = x[order]
    with np.errstate(invalid="ignore", over="ignore"):
        out[:, time_col] = out[:, time_col] - tmin
        if charge_col < 0:
            out[:, F] = 1.0
        else:
            out[:, charge_col] = np.power(10.0, out[:, charge_col].astype(np.float64)).astype(np.float32)
    ids = np.stack(keys[1:], axis=1)[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (ids[1:] != ids[:-1]).any(axis=1)
    out[:, W - 1] = head
    return out


class NodeAsDOMTimeSeries(NodeDefinition):
    """The pulses of an event regrouped into one time series per DOM (``nodes/nodes.py:220-306``; argument names, order
    and defaults are the reference's): rows grouped by ``id_columns``, ascending in time inside a group, the time shifted
    to start at 0, the charge raised to ``10^x`` (undoing the detector's ``log10``) and a last column ``new_node_col``
    that is 1 on every group's first row.  The row count does not change.  The arithmetic is defined operation by
    operation in ``include/graphnet_amd.h`` (``gn_dom_time_series``).  A device tensor takes one ``gn_dom_time_series``
    call; a CPU tensor takes :func:`dom_time_series_host`, the same contract in numpy.  On the device a whole batch is
    regrouped by one call: ``GraphDefinition.batch_from_raw``, whose batch also carries ``series_ptr`` / ``dom_ptr``.

    ``charge_column`` naming no feature (the example's ``"None"``) runs without: a column of ones (``10^0``) is appended
    before ``new_node_col``, and the output NAMES are still ``input_feature_names + ["new_node_col"]`` as in the reference
    (``nb_outputs`` counts the names; the matrix is one wider).

    ``max_activations`` is stored and never used, exactly as in the reference (``nodes.py:261``; nothing reads it).

    One definition where the reference has none: its ``argsort`` on time is not stable, so the order among pulses of one
    DOM with equal times is arbitrary there; here it is the original pulse order.
    """

    def __init__(self, keys: List[str] = ["dom_x", "dom_y", "dom_z", "dom_time", "charge"],
                 id_columns: List[str] = ["dom_x", "dom_y", "dom_z"], time_column: str = "dom_time",
                 charge_column: str = "charge", max_activations: Optional[int] = None) -> None:
        self._keys = list(keys)
        super().__init__(input_feature_names=self._keys)
        self._id_columns = [self._keys.index(key) for key in id_columns]
        self._time_index = self._keys.index(time_column)
        self._charge_index: Optional[int] = self._keys.index(charge_column) if charge_column in self._keys else None
        self._max_activations = max_activations

    def _define_output_feature_names(self, input_feature_names: List[str]) -> List[str]:
        return input_feature_names + ["new_node_col"]

    def series_batch(self, x: torch.Tensor, ptr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(rows fp32 [N, W], series_ptr int32 [M + 1], dom_ptr int32 [B + 1])`` of the events ``ptr`` marks in ``x``:
        one device call, or the host path event by event for a CPU tensor."""
        charge = -1 if self._charge_index is None else self._charge_index
        if x.is_cuda:
            from . import ops
            return ops.dom_time_series(x.to(torch.float32), ptr.to(torch.int32), self._id_columns, self._time_index, charge)
        xn, bounds = x.detach().to(torch.float32).numpy(), ptr.tolist()
        parts = [dom_time_series_host(xn[lo:hi], self._id_columns, self._time_index, charge)
                 for lo, hi in zip(bounds[:-1], bounds[1:])]
        W = int(x.shape[1]) + (1 if charge < 0 else 0) + 1
        rows = np.concatenate(parts, axis=0) if parts else np.zeros((0, W), dtype=np.float32)
        series_ptr = np.append(np.flatnonzero(rows[:, -1]), len(rows)).astype(np.int32)
        dom_ptr = np.zeros(len(bounds), dtype=np.int32)
        dom_ptr[1:] = np.cumsum([int(p[:, -1].sum()) for p in parts])
        return torch.from_numpy(rows), torch.from_numpy(series_ptr), torch.from_numpy(dom_ptr)

    def _construct_nodes(self, x: torch.Tensor) -> Data:
        ptr = torch.tensor([0, int(x.shape[0])], dtype=torch.int32, device=x.device)
        return Data(x=self.series_batch(x, ptr)[0])

_M32 = np.uint64(0xFFFFFFFF)


def _mix32(v: np.ndarray) -> np.ndarray:
    """``gn_mix32`` of ``graphnet_amd/csrc/common.hpp`` on uint32 values held in uint64 arrays."""
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x21F0AAAD)) & _M32
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x735A2D97)) & _M32
    return v ^ (v >> np.uint64(15))


def icemix_keys(seed: int, event_id: int, n: int, key_bits: int = 32) -> np.ndarray:
    """The sampling key of every pulse of one event (``gn_icemix_nodes``): uint64 ``[n]`` holding uint32 values."""
    stream = _mix32(np.uint64(seed & 0xFFFFFFFF) ^ ((np.uint64(event_id & 0xFFFFFFFF) * np.uint64(0x9E3779B1)) & _M32))
    i = np.arange(n, dtype=np.uint64)
    return _mix32(stream ^ ((i * np.uint64(0x85EBCA77)) & _M32)) >> np.uint64(32 - key_bits)


def ice_table_host(depth: np.ndarray, scattering_len: np.ndarray, absorption_len: np.ndarray,
                   z_offset: Optional[float] = None, z_scaling: Optional[float] = None) -> np.ndarray:
    """What the reference's ``ice_transparency`` (``models/graphs/utils.py:175-209``) builds its two ``interp1d``
    functions from, as fp64 ``[3, T]``: the knots ``(depth + (z_offset or -1950)) / (z_scaling or 500)`` ascending, then both
    lengths through sklearn's ``RobustScaler`` - ``(v - median) / (q75 - q25)``, which is all that scaler does to one
    column, in numpy alone."""
    z = (np.asarray(depth, dtype=np.float64) + (z_offset or -1950.0)) / (z_scaling or 500.0)
    cols = [z]
    for v in (scattering_len, absorption_len):
        v = np.asarray(v, dtype=np.float64)
        cols.append((v - np.median(v)) / (np.percentile(v, 75) - np.percentile(v, 25)))
    table = np.stack(cols)[:, np.argsort(z, kind="stable")]           # interp1d sorts its knots
    if table.shape[1] < 2 or not (np.diff(table[0]) > 0).all():
        raise ValueError("ice table: need at least two rows and distinct depths")
    return np.ascontiguousarray(table)


def ice_interp_host(table: np.ndarray, z: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Both ice functions at the fp32 depths ``z``, in fp64 (the contract of ``gn_icemix_nodes``: interval ``j`` = the largest
    index with ``zt[j] <= z``, at most ``T - 2``; ``slope = (y[j+1] - y[j]) / (zt[j+1] - zt[j])``; ``slope * (z - zt[j]) + y[j]``).
    A depth outside the table, or NaN, raises ``ValueError`` as the reference's ``interp1d`` does."""
    zt = table[0]
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    if not ((z >= zt[0]) & (z <= zt[-1])).all():
        raise ValueError(f"A value in the z column is outside the interpolation range [{zt[0]}, {zt[-1]}] of the ice table")
    j = np.clip(np.searchsorted(zt, z, side="right") - 1, 0, len(zt) - 2)
    dz, t = zt[j + 1] - zt[j], z - zt[j]
    return tuple(((y[j + 1] - y[j]) / dz) * t + y[j] for y in (table[1], table[2]))


def icemix_nodes_host(x: np.ndarray, ptr: np.ndarray, max_pulses: int, hlc_col: int = -1, z_col: int = -1,
                      table: Optional[np.ndarray] = None, seed: int = 0, event_ids: Optional[np.ndarray] = None,
                      key_bits: int = 32) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The contract of ``gn_icemix_nodes`` (``include/graphnet_amd.h``) for a whole batch in vectorised numpy: fp32
    ``[N, F]`` -> ``(nodes fp32 [M, F + 2*(z_col >= 0)], node_ptr int32 [B + 1], ids int32 [M])``.  Bit for bit what the
    kernel writes, but that a depth outside the ice table raises ``ValueError`` here and is NaN there."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bounds = np.asarray(ptr, dtype=np.int64)
    L, B, F = int(max_pulses), len(bounds) - 1, x.shape[1]
    kept = []
    for b in range(B):
        lo, n = int(bounds[b]), int(bounds[b + 1] - bounds[b])
        if n <= L:
            kept.append(lo + np.arange(n, dtype=np.int64))
        else:       # the L smallest in the total order (key, index), then back in pulse order
            h = icemix_keys(seed, b if event_ids is None else int(event_ids[b]), n, key_bits)
            kept.append(lo + np.sort(np.argsort(h, kind="stable")[:L]))
    node_ptr = np.zeros(B + 1, dtype=np.int32)
    node_ptr[1:] = np.cumsum([len(k) for k in kept])
    ids = np.concatenate(kept).astype(np.int32) if kept else np.zeros(0, dtype=np.int32)
    out = np.zeros((len(ids), F + (2 if z_col >= 0 else 0)), dtype=np.float32)
    out[:, :F] = x[ids]
    if hlc_col >= 0:
        out[:, hlc_col] = x[ids, hlc_col] == 0
    if z_col >= 0:
        out[:, F], out[:, F + 1] = ice_interp_host(table, x[ids, z_col])
    return out, node_ptr, ids


def _read_ice_table(path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    names = ("depth", "scattering_len", "absorption_len")
    if path.endswith(".npz"):
        d = np.load(path)
        return tuple(np.asarray(d[k], dtype=np.float64) for k in names)
    import pandas as pd
    df = pd.read_parquet(path)
    return tuple(np.asarray(df[k], dtype=np.float64) for k in names)


def _find_ice_table() -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    path = os.environ.get("GRAPHNET_AMD_ICE_TABLE")
    if path:
        return _read_ice_table(path)
    try:
        from graphnet.constants import DATA_DIR
    except Exception:
        DATA_DIR = None
    if DATA_DIR is not None:
        return _read_ice_table(os.path.join(DATA_DIR, "ice_properties", "ice_transparency.parquet"))
    raise RuntimeError(
        "IceMixNodes(add_ice_properties=True) needs the ice transparency table, which this package does not ship: set "
        "$GRAPHNET_AMD_ICE_TABLE to the reference's data/ice_properties/ice_transparency.parquet (or an .npz with the "
        "columns depth, scattering_len, absorption_len), assign IceMixNodes.ice_table = (depth, scattering_len, "
        "absorption_len) before constructing (or on an instance, to replace its table), or install graphnet, whose "
        "DATA_DIR is then used")


class IceMixNodes(NodeDefinition):
    """Ice properties and random pulse sampling (``nodes/nodes.py:309-453``; argument names, order and defaults are the
    reference's, ``scatt_lenght`` / ``abs_lenght`` are its spelling).  Per event: the ``hlc_name`` column becomes its
    logical not, an event of more than ``max_pulses`` pulses keeps ``max_pulses`` of them, and with
    ``add_ice_properties`` two columns are appended: the scattering and absorption length of the ice at the pulse's
    ``z_name``, linear interpolation in fp64 of the reference's table after ``RobustScaler``.  The arithmetic is defined
    operation by operation in ``include/graphnet_amd.h`` (``gn_icemix_nodes``).  A device tensor takes one
    ``gn_icemix_nodes`` call; a CPU tensor takes :func:`icemix_nodes_host`, the same contract in numpy, ids and rows bit
    for bit.  On the device a whole batch is sampled by one call: ``GraphDefinition.batch_from_raw``, whose batch also
    carries ``pulse_ids``.

    **Which pulses are kept.**  A uniformly random ``max_pulses``-subset of the event, in pulse order, whatever the hlc
    column holds.  That is the reference's distribution: it draws ``ids = randperm(n)`` and takes ``ids[auxiliary_n]`` and
    ``ids[auxiliary_p]`` - the PERMUTATION at the positions of the flagged pulses, not the flagged pulses - so the two
    parts are disjoint random ids unrelated to hlc, and their sorted union is a uniform subset.  There is no hlc-priority
    option here either.  The subset is a function of ``(seed, event id, pulse index)`` through the library's counter
    hash, not torch's generator stream.  One definition where the reference differs: with ``hlc_name=None`` it keeps
    the subset in random order; here the rows are always in pulse order.

    **The ice table** is data of the reference and is not shipped: it is read from ``$GRAPHNET_AMD_ICE_TABLE`` (the
    reference's parquet, or an ``.npz`` with the columns ``depth``, ``scattering_len``, ``absorption_len``), taken from
    ``ice_table`` when that was assigned (on the class before construction, or on an instance to replace its table), or
    read from the reference's ``DATA_DIR`` when ``graphnet`` is importable; otherwise construction with
    ``add_ice_properties=True`` raises.  A z outside the table raises ``ValueError`` on the host, as in the reference; the
    kernel cannot raise and writes NaN into both ice columns."""

    ice_table: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]] = None

    def __init__(self, input_feature_names: Optional[List[str]] = None, max_pulses: int = 768, z_name: str = "dom_z",
                 hlc_name: Optional[str] = "hlc", add_ice_properties: bool = True,
                 ice_args: Dict[str, Optional[float]] = {"z_offset": None, "z_scaling": None}) -> None:
        if input_feature_names is None:
            input_feature_names = ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "hlc", "rde"]
        input_feature_names = list(input_feature_names)
        if add_ice_properties:
            if z_name not in input_feature_names:
                raise ValueError(f"z name '{z_name}' not found in input_feature_names {input_feature_names}")
            self.all_features = input_feature_names + ["scatt_lenght", "abs_lenght"]
            if self.ice_table is None:
                self.ice_table = _find_ice_table()
        else:
            self.all_features = input_feature_names
        self._ice_args = dict(ice_args)
        self._table_cache: Dict[Any, Any] = {}
        super().__init__(input_feature_names=input_feature_names)
        if hlc_name not in input_feature_names:
            warnings.warn(f"hlc name '{hlc_name}' not found in input_feature_names '{input_feature_names}', "
                          "subsampling will be random.")
            hlc_name = None
        self.feature_indexes = {feat: self.all_features.index(feat) for feat in input_feature_names}
        self.input_feature_names = input_feature_names
        self.n_features = len(self.all_features)
        self.max_length = max_pulses
        self.z_name = z_name
        self.hlc_name = hlc_name
        self.add_ice_properties = add_ice_properties

    def _define_output_feature_names(self, input_feature_names: List[str]) -> List[str]:
        return self.all_features

    def _table(self, device: Any = None) -> Any:
        """fp64 ``[3, T]`` of :func:`ice_table_host` for the present ``ice_table`` (numpy, or a tensor on ``device``)."""
        if self._table_cache.get("source") is not self.ice_table:
            self._table_cache = {"source": self.ice_table, None: ice_table_host(*self.ice_table, **self._ice_args)}
        if device not in self._table_cache:
            self._table_cache[device] = torch.from_numpy(self._table_cache[None]).to(device)
        return self._table_cache[device]

    def f_scattering(self, z: Any) -> np.ndarray:
        return ice_interp_host(self._table(), np.asarray(z))[0]

    def f_absoprtion(self, z: Any) -> np.ndarray:
        return ice_interp_host(self._table(), np.asarray(z))[1]

    def sample_batch(self, x: torch.Tensor, ptr: torch.Tensor, seed: Optional[int] = None,
                     event_ids: Optional[Any] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(nodes fp32 [M, n_features], node_ptr int32 [B + 1], ids int32 [M])`` of the events ``ptr`` marks in ``x``;
        ``ids`` is the row of ``x`` behind every node.  One device call, or the host path for a CPU tensor.  ``seed=None``
        draws one uint32 from torch's global CPU generator, so ``torch.manual_seed`` reproduces a run and successive calls
        differ; ``event_ids`` (``[B]`` integers, by default the ordinals) name the stream of each event."""
        if seed is None:
            seed = int(torch.randint(0, 2 ** 32, (1,), dtype=torch.int64).item())
        hlc = -1 if self.hlc_name is None else self.feature_indexes[self.hlc_name]
        z = self.feature_indexes[self.z_name] if self.add_ice_properties else -1
        if x.is_cuda:
            from . import ops
            ev = None if event_ids is None else torch.as_tensor(event_ids)
            return ops.icemix_nodes(x.to(torch.float32), ptr.to(torch.int32), self.max_length, hlc, z,
                                    self._table(x.device) if z >= 0 else None, seed, ev)
        ev = None if event_ids is None else np.asarray(torch.as_tensor(event_ids).cpu().numpy(), dtype=np.int64)
        nodes, node_ptr, ids = icemix_nodes_host(x.detach().to(torch.float32).numpy(), ptr.cpu().numpy(), self.max_length, hlc,
                                                 z, self._table() if z >= 0 else None, seed, ev)
        return torch.from_numpy(nodes), torch.from_numpy(node_ptr), torch.from_numpy(ids)

    def _construct_nodes(self, x: torch.Tensor) -> Data:
        ptr = torch.tensor([0, int(x.shape[0])], dtype=torch.int32, device=x.device)
        return Data(x=self.sample_batch(x, ptr)[0])


class EdgeDefinition(Model):
    def forward(self, graph: Data) -> Data:
        return self._construct_edges(graph)


class KNNEdges(EdgeDefinition):
    """k-nearest-neighbour edges in the space of ``columns`` (``edges.py:47-80``)."""

    def __init__(self, nb_nearest_neighbours: int, columns: List[int] = [0, 1, 2]):
        super().__init__()
        self._nb_nearest_neighbours = nb_nearest_neighbours
        self._columns = list(columns)

    def _construct_edges(self, graph: Data) -> Data:
        x = graph.x
        if x.is_cuda:
            from . import ops
            n = int(x.shape[0])
            batch = getattr(graph, "batch", None) if "batch" in graph else None
            if batch is None:
                ptr = torch.tensor([0, n], dtype=torch.int32, device=x.device)
                batch32 = torch.zeros(n, dtype=torch.int32, device=x.device)
            else:
                batch32 = batch.to(torch.int32)
                counts = torch.bincount(batch)
                ptr = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=x.device)
                ptr[1:] = torch.cumsum(counts, 0)
            table = ops.knn_graph(x.to(torch.float32), self._columns, batch32, ptr, self._nb_nearest_neighbours, sweep=True)
            graph.edge_index = table.edge_index()
        else:
            graph.edge_index = None            # built on device for the whole batch by the backbone
        graph.knn_k = self._nb_nearest_neighbours
        graph.knn_columns = list(self._columns)
        return graph


def _event_ptr(x: torch.Tensor, batch: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(batch32, ptr32)`` of a device graph: one event when it carries no ``batch``."""
    n = int(x.shape[0])
    if batch is None:
        return (torch.zeros(n, dtype=torch.int32, device=x.device),
                torch.tensor([0, n], dtype=torch.int32, device=x.device))
    counts = torch.bincount(batch)
    ptr = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=x.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return batch.to(torch.int32), ptr


# what MinkowskiKNNEdges records on a graph it does not build at once: scalars + one list, as knn_k / knn_columns are,
# so that Batch.from_data_list / collate_fn / select_events / .to(device) carry them without knowing them
MINKOWSKI_RECORD = ("mink_k", "mink_c", "mink_time_like_weight", "mink_time_coord", "mink_space_coords")


def minkowski_record(data: Any) -> Optional[Tuple[int, float, float, int, List[int]]]:
    """``(k, c, time_like_weight, time_coord, space_coords)`` recorded by :class:`MinkowskiKNNEdges` on ``data`` (a
    ``Data``, or a ``Batch`` where the scalars have become ``[B]`` tensors and the list a list of lists), or None."""
    def get(name: str) -> Any:
        try:
            return data[name] if name in data else None
        except TypeError:                                   # an object without __contains__ / __getitem__
            return getattr(data, name, None)

    def scalar(v: Any) -> Any:
        return v.reshape(-1)[0].item() if isinstance(v, torch.Tensor) else v

    k = get("mink_k")
    if k is None:
        return None
    sc = get("mink_space_coords")
    sc = list(sc[0]) if isinstance(sc, list) and sc and isinstance(sc[0], (list, tuple)) else list(sc)
    return (int(scalar(k)), float(scalar(get("mink_c"))), float(scalar(get("mink_time_like_weight"))),
            int(scalar(get("mink_time_coord"))), [int(v) for v in sc])


class MinkowskiKNNEdges(EdgeDefinition):
    """Edges to the ``nb_nearest_neighbours`` most light-like separated pulses of the same event
    (``graphs/edges/minkowski.py:37-99``; argument names, order, defaults and public attributes are the reference's).

    For centre ``i`` and every other pulse ``j`` of its event, in fp32 without FMA contraction::

        sp = ((0 + d0*d0) + d1*d1) + ...      over space_coords, left to right
        tc = (t_i - t_j) * c ;  m = sp - tc*tc
        if m < 0: m = m * (-time_like_weight)

    and the ``k`` smallest in the total order ``(m, j)`` become the edges ``j -> i`` (``edge_index[0] = j``,
    ``edge_index[1] = i``, grouped by ``i``, ascending ``(m, j)``): degree ``min(k, n - 1)``, no self loops, a pulse
    with a NaN ``m`` (or ``m >= 3.0e38``) is nobody's neighbour.  One ``gn_minkowski_knn_graph`` launch for the whole
    batch; on a CPU ``Data`` the parameters are recorded (``MINKOWSKI_RECORD``) and the backbone builds the graph.

    Two deliberate differences from the reference's literal text:

    * **Row slice vs column slice.**  ``minkowski.py:93`` takes ``distance_sorted[:num_edges]``, the first k ROWS of
      the per-row argsort, where "the k nearest of every centre" needs its first k COLUMNS; the reference's own test
      only accepts that through an ``or`` branch that compares targets with themselves.  This class builds the
      per-centre meaning (as ``oracle/knn_oracle.c`` does).
    * **Tie order.**  The reference's order among equal ``m`` is whatever ``argsort`` returns; here it is ``(m, j)``.
      The centre is excluded by index, not by adding 1e9 to the diagonal.
    """

    def __init__(self, nb_nearest_neighbours: int, c: float, time_like_weight: float = 1.0,
                 space_coords: Optional[List[int]] = None, time_coord: Optional[int] = 3):
        super().__init__()
        self.nb_nearest_neighbours = nb_nearest_neighbours
        self.c = c
        self.time_like_weight = time_like_weight
        self.space_coords = space_coords or [0, 1, 2]
        self.time_coord = time_coord

    def _record(self, graph: Data) -> Data:
        graph.mink_k = int(self.nb_nearest_neighbours)
        graph.mink_c = float(self.c)
        graph.mink_time_like_weight = float(self.time_like_weight)
        graph.mink_time_coord = int(self.time_coord)
        graph.mink_space_coords = [int(v) for v in self.space_coords]
        return graph

    def _construct_edges(self, graph: Data) -> Data:
        x = graph.x
        if x.is_cuda:
            from . import ops
            batch32, ptr = _event_ptr(x, getattr(graph, "batch", None) if "batch" in graph else None)
            table = ops.minkowski_knn_graph(x.to(torch.float32), self.space_coords, self.time_coord, self.c,
                                            self.time_like_weight, batch32, ptr, self.nb_nearest_neighbours)
            graph.edge_index = table.edge_index()
        else:
            graph.edge_index = None            # built on device for the whole batch by the backbone
        return self._record(graph)


# what RadialEdges records on a graph it does not build at once (same construction as MINKOWSKI_RECORD)
RADIAL_RECORD = ("radial_r", "radial_columns", "radial_max")


def radial_record(data: Any) -> Optional[Tuple[float, List[int], int]]:
    """``(radius, columns, max_num_neighbours)`` recorded by :class:`RadialEdges` on ``data`` (a ``Data``, or a ``Batch``
    where the scalars have become ``[B]`` tensors and the list a list of lists), or None."""
    def get(name: str) -> Any:
        try:
            return data[name] if name in data else None
        except TypeError:                                   # an object without __contains__ / __getitem__
            return getattr(data, name, None)

    def scalar(v: Any) -> Any:
        return v.reshape(-1)[0].item() if isinstance(v, torch.Tensor) else v

    r = get("radial_r")
    if r is None:
        return None
    cols = get("radial_columns")
    cols = list(cols[0]) if isinstance(cols, list) and cols and isinstance(cols[0], (list, tuple)) else list(cols)
    return float(scalar(r)), [int(v) for v in cols], int(scalar(get("radial_max")))


class RadialEdges(EdgeDefinition):
    """Edges from every pulse of the same event inside a sphere of ``radius`` around each pulse, in the space of
    ``columns`` (``graphs/edges/edges.py:83-117``; the first two arguments carry the reference's names, order and
    defaults, the third exposes what the reference leaves at ``radius_graph``'s default ``max_num_neighbors = 32``).

    For centre ``i`` and every other pulse ``j`` of its event, in fp32 without FMA contraction::

        d2 = ((0 + e0*e0) + e1*e1) + ...      e = x[j, col] - x[i, col], columns left to right
        r2 = r * r                            one fp32 multiply of the fp32-rounded radius
        edge j -> i   iff   j != i  and  d2 < r2        (strict)

    ``edge_index[0] = j``, ``edge_index[1] = i``, grouped by ``i``, ascending ``j`` inside a group; no self loops; a
    pulse with a NaN or inf coordinate has no neighbours and is nobody's neighbour.  One ``gn_radius_graph`` call for
    the whole batch; on a CPU ``Data`` the parameters are recorded (``RADIAL_RECORD``) and the backbone builds the
    graph.  At most 32 neighbours per centre: that is the width of the edge kernels.

    One deliberate difference from the reference:

    * **Which neighbours survive the cap.**  Where more than ``max_num_neighbours`` pulses lie inside the radius,
      ``torch_cluster`` keeps whichever its scan or tree meets first - a choice that depends on the storage order of the
      pulses and differs between its CPU and CUDA builds.  Here the kept ones are the ``max_num_neighbours`` smallest in
      the total order ``(d2, j)``, which does not depend on the order of the pulses; they are still stored ascending
      by ``j``.  Wherever no centre exceeds the cap the edge set is that of any ``radius_graph``.
    """

    def __init__(self, radius: float, columns: List[int] = [0, 1, 2], max_num_neighbours: int = 32):
        super().__init__()
        self._radius = radius
        self._columns = list(columns)
        self._max_num_neighbours = max_num_neighbours

    def _record(self, graph: Data) -> Data:
        graph.radial_r = float(self._radius)
        graph.radial_columns = [int(v) for v in self._columns]
        graph.radial_max = int(self._max_num_neighbours)
        return graph

    def _construct_edges(self, graph: Data) -> Data:
        x = graph.x
        if x.is_cuda:
            from . import ops
            batch32, ptr = _event_ptr(x, getattr(graph, "batch", None) if "batch" in graph else None)
            table = ops.radius_graph(x.to(torch.float32), self._columns, self._radius, batch32, ptr,
                                     self._max_num_neighbours)
            graph.edge_index = table.edge_index()
        else:
            graph.edge_index = None            # built on device for the whole batch by the backbone
        return self._record(graph)


class GraphDefinition(Model):
    """numpy pulses -> ``Data`` (``models/graphs/graph_definition.py:27-465``): optional inactive sensors, sensor /
    string masks and Gaussian perturbation on the raw array, then tensor -> detector standardisation -> node
    definition -> optional sort -> ``n_pulses`` -> edges -> loss weight, truth / custom labels (optionally repeated
    per node) and the node features as separate attributes."""

    def __init__(
        self,
        detector: Detector,
        node_definition: Optional[NodeDefinition] = None,
        edge_definition: Optional[EdgeDefinition] = None,
        input_feature_names: Optional[List[str]] = None,
        dtype: Optional[torch.dtype] = torch.float,
        perturbation_dict: Optional[Dict[str, float]] = None,
        seed: Optional[Union[int, Generator]] = None,
        add_inactive_sensors: bool = False,
        sensor_mask: Optional[List[int]] = None,
        string_mask: Optional[List[int]] = None,
        sort_by: Optional[str] = None,
        repeat_labels: bool = False,
    ):
        super().__init__()
        self._detector = detector
        self._node_definition = node_definition or NodesAsPulses()
        self._edge_definition = edge_definition
        self._perturbation_dict = perturbation_dict
        self._add_inactive_sensors = add_inactive_sensors
        self._repeat_labels = repeat_labels
        # one of the two masks at most; a string mask becomes the list of sensor ids on those strings
        assert sensor_mask is None or string_mask is None, \
            "Got arguments for both `sensor_mask` and `string_mask`. Please specify only one."
        if string_mask is not None:
            table = detector.geometry_table
            on_string = table[detector.string_index_name].isin(string_mask)
            sensor_mask = np.asarray(table.loc[on_string, detector.sensor_index_name]).tolist()
        self._sensor_mask, self._string_mask = sensor_mask, string_mask
        if input_feature_names is None:
            input_feature_names = list(detector.feature_map().keys())
        self._input_feature_names = list(input_feature_names)
        self._node_definition.set_number_of_inputs(self._input_feature_names)
        self._node_definition.set_output_feature_names(self._input_feature_names)
        self.output_feature_names = list(getattr(self._node_definition, "_output_feature_names",
                                                 self._input_feature_names))
        self._sort_by = None
        if sort_by is not None:
            assert isinstance(sort_by, str)
            self._sort_by = self.output_feature_names.index(sort_by)       # ValueError if it is not a node feature
        self.nb_inputs = len(self._input_feature_names)
        self.nb_outputs = self._node_definition.nb_outputs
        self.dtype = dtype
        if isinstance(self._perturbation_dict, dict):
            self._perturbation_cols = [self._input_feature_names.index(k) for k in self._perturbation_dict]
        if isinstance(seed, Generator):
            self.rng = seed
        elif seed is None:
            self.rng = default_rng()
        elif isinstance(seed, int):
            self.rng = default_rng(seed)
        else:
            raise ValueError("Invalid seed. Must be an int or a numpy Generator.")
        self._sensor_rows: Optional[Dict[Tuple[float, ...], int]] = None

    # ---- geometry-table helpers (graph_definition.py:263-325) ------------------------------------------------
    def _geometry_rows(self, input_features: np.ndarray, input_feature_names: List[str]) -> np.ndarray:
        """Row of the detector's geometry table for every pulse, looked up by its xyz position (KeyError for a
        position that is not in the table, as the reference's ``.loc`` lookup)."""
        det = self._detector
        if self._sensor_rows is None:
            pos = det.geometry_table.reset_index()[det.sensor_position_names].to_numpy(dtype=np.float64)
            self._sensor_rows = {tuple(row): i for i, row in enumerate(pos.tolist())}
        cols = [input_feature_names.index(f) for f in det.sensor_position_names]
        keys = np.asarray(input_features[:, cols], dtype=np.float64).tolist()
        return np.fromiter((self._sensor_rows[tuple(k)] for k in keys), dtype=np.int64, count=len(keys))

    def _attach_inactive_sensors(self, input_features: np.ndarray, input_feature_names: List[str]) -> np.ndarray:
        """Append one padded row per sensor of the geometry table that recorded no pulse."""
        table = self._detector.geometry_table.reset_index()
        hit = np.zeros(len(table), dtype=bool)
        hit[self._geometry_rows(input_features, input_feature_names)] = True
        missing = [f for f in input_feature_names if f not in table.columns]
        if missing:
            raise KeyError(f"geometry table lacks the columns {missing} needed to pad inactive sensors")
        inactive = table.loc[~hit, input_feature_names].to_numpy()
        return np.concatenate([input_features, inactive], axis=0)

    def _mask_sensors(self, input_features: np.ndarray, input_feature_names: List[str]) -> np.ndarray:
        """Drop the pulses recorded by a masked sensor."""
        table = self._detector.geometry_table.reset_index()
        ids = table[self._detector.sensor_index_name].to_numpy()[self._geometry_rows(input_features, input_feature_names)]
        return input_features[~np.isin(ids, np.asarray(self._sensor_mask)), :]

    def _validate_input(self, input_features: np.ndarray, input_feature_names: List[str]) -> None:
        assert input_features.shape[1] == len(input_feature_names)
        assert list(input_feature_names) == self._input_feature_names, (
            f"Input features ({input_feature_names}) is not what {self.__class__.__name__} was "
            f"instantiated with ({self._input_feature_names})")

    def _perturb_input(self, input_features: np.ndarray) -> np.ndarray:
        if isinstance(self._perturbation_dict, dict):
            sig = np.array(list(self._perturbation_dict.values()), dtype=float)
            input_features[:, self._perturbation_cols] = self.rng.normal(
                loc=input_features[:, self._perturbation_cols], scale=sig)
        return input_features

    def _add_loss_weights(self, graph: Data, loss_weight_column: Optional[str], loss_weight: Optional[float],
                          loss_weight_default_value: Optional[float]) -> Data:
        """``graph[loss_weight_column] = loss_weight`` as a ``[1, 1]`` tensor; a negative weight means "missing"
        and takes the default value (``graph_definition.py:363-398``; the reference reads the default from an
        attribute it never sets - the argument is used here)."""
        if loss_weight is not None and loss_weight_column is not None:
            if loss_weight < 0:
                if loss_weight_default_value is None:
                    raise ValueError(f"At least one event is missing an entry in {loss_weight_column} "
                                     "but loss_weight_default_value is None.")
                loss_weight = loss_weight_default_value
            graph[loss_weight_column] = torch.tensor(loss_weight, dtype=self.dtype).reshape(-1, 1)
        return graph

    def _label(self, value: Any, graph: Data) -> torch.Tensor:
        label = value if isinstance(value, torch.Tensor) else torch.tensor(value)
        return label.repeat(graph.x.shape[0], 1) if self._repeat_labels else label

    def forward(self, input_features: np.ndarray, input_feature_names: List[str],
                truth_dicts: Optional[List[Dict[str, Any]]] = None,
                custom_label_functions: Optional[Dict[str, Callable[..., Any]]] = None,
                loss_weight_column: Optional[str] = None, loss_weight: Optional[float] = None,
                loss_weight_default_value: Optional[float] = None, data_path: Optional[str] = None) -> Data:
        self._validate_input(input_features, input_feature_names)
        if self._add_inactive_sensors:
            input_features = self._attach_inactive_sensors(input_features, input_feature_names)
        if self._sensor_mask is not None:
            input_features = self._mask_sensors(input_features, input_feature_names)
        input_features = self._perturb_input(input_features)
        x = torch.tensor(input_features, dtype=self.dtype)
        x = self._detector(x, input_feature_names)
        graph, node_feature_names = self._node_definition(x)
        if self._sort_by is not None:
            graph.x = graph.x[graph.x[:, self._sort_by].sort()[1]]
        graph.x = graph.x.type(self.dtype)
        graph.n_pulses = torch.tensor(len(input_features), dtype=torch.int32)
        if self._edge_definition is not None:
            graph = self._edge_definition(graph)
        if data_path is not None:
            graph["dataset_path"] = data_path
        graph = self._add_loss_weights(graph, loss_weight_column, loss_weight, loss_weight_default_value)
        if truth_dicts is not None:
            for td in truth_dicts:
                for k, v in td.items():
                    try:
                        graph[k] = self._label(v, graph)
                    except (TypeError, ValueError, RuntimeError):      # e.g. a string: not attached (as the reference)
                        pass
        if custom_label_functions is not None:
            for k, fn in custom_label_functions.items():
                graph[k] = self._label(fn(graph), graph)
        # the node features once more as separate attributes ('x' is reserved for the feature matrix)
        names = list(node_feature_names) if node_feature_names is not None else list(self.output_feature_names)
        graph["features"] = names
        for index, feature in enumerate(names):
            if feature != "x":
                graph[feature] = graph.x[:, index].detach()
        graph["graph_definition"] = self.__class__.__name__
        return graph


def _batch_from_raw(self: "GraphDefinition", events: "List[np.ndarray]", input_feature_names: "List[str]",
                    truth: "Optional[Dict[str, Any]]" = None, device: str = "cuda") -> "Batch":
    """Device-side replacement of the per-event loader path (``data/dataset/dataset.py:591-652`` +
    ``data/dataloader.py:12-18``): raw pulse arrays of many events -> ONE flat ``[N, F]`` buffer + ``ptr`` -> one
    host-to-device copy -> the detector's standardisation as one kernel over the whole batch
    (``gn_standardize``, bit-identical to the per-event host expressions) -> ``Batch`` without edges (the backbone
    builds the layer-1 k-NN on device, ``gn_knn_graph``).  Events with <= 1 pulse are dropped, as ``collate_fn``
    does.  With a :class:`PercentileClusters` node definition the standardised batch goes through one
    ``gn_percentile_clusters`` call: ``x`` / ``ptr`` / ``batch`` describe the clusters, ``n_pulses`` the raw pulses.
    With a :class:`NodeAsDOMTimeSeries` node definition it goes through one ``gn_dom_time_series`` call: the rows stay
    pulses (``x`` / ``ptr`` / ``batch`` / ``n_pulses``), and the batch also carries ``series_ptr`` / ``dom_ptr``.
    With an :class:`IceMixNodes` node definition it goes through one ``gn_icemix_nodes`` call: ``x`` / ``ptr`` / ``batch``
    describe the kept pulses, ``n_pulses`` the raw pulses, and ``pulse_ids`` names the row of the standardised batch behind
    every kept pulse (for truth per pulse).
    ``truth``: name -> per-event sequence (filtered alongside)."""
    from .data import Batch
    keep = [i for i, e in enumerate(events) if len(e) > 1]
    sizes = np.asarray([len(events[i]) for i in keep], dtype=np.int64)
    ptr = np.zeros(len(keep) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(sizes)
    flat = torch.empty((int(ptr[-1]), len(input_feature_names)), dtype=self.dtype,
                       pin_memory=torch.cuda.is_available() and device != "cpu")
    flat_np = flat.numpy()
    for j, i in enumerate(keep):
        ev = np.asarray(events[i])
        self._validate_input(ev, input_feature_names)
        flat_np[ptr[j]:ptr[j + 1]] = self._perturb_input(ev.copy() if self._perturbation_dict else ev)
    x = flat.to(device, non_blocking=True)
    x = self._detector(x, input_feature_names)
    if self._sort_by is not None:
        raise NotImplementedError("graphnet_amd: sort_by is a per-event host option; use the per-event path")
    nd = self._node_definition
    n_pulses = torch.from_numpy(sizes).to(torch.int32)
    if isinstance(nd, PercentileClusters):
        # one clustering call over the whole batch: ptr / batch describe nodes from here on, n_pulses stays pulses
        nodes, node_ptr = nd.cluster_batch(x, torch.from_numpy(ptr).to(torch.int32).to(x.device))
        b = Batch(x=nodes.type(self.dtype))
        b.ptr = node_ptr.to(torch.int64)
        b.n_pulses = n_pulses.to(device)
        b.batch = torch.repeat_interleave(torch.arange(len(keep), dtype=torch.int64, device=b.ptr.device),
                                          b.ptr[1:] - b.ptr[:-1], output_size=int(nodes.shape[0]))
    elif isinstance(nd, NodesAsPulses):
        b = Batch(x=x)
        ptr_t = torch.from_numpy(ptr)
        b.ptr = ptr_t.to(device)
        b.n_pulses = n_pulses.to(device)
        b.batch = torch.repeat_interleave(torch.arange(len(keep), dtype=torch.int64), torch.from_numpy(sizes)).to(device)
    elif isinstance(nd, NodeAsDOMTimeSeries):
        # one regrouping call over the whole batch: the rows stay pulses, series_ptr / dom_ptr mark the DOM series
        rows, series_ptr, dom_ptr = nd.series_batch(x, torch.from_numpy(ptr).to(torch.int32).to(x.device))
        b = Batch(x=rows.type(self.dtype))
        b.ptr = torch.from_numpy(ptr).to(device)
        b.n_pulses = n_pulses.to(device)
        b.batch = torch.repeat_interleave(torch.arange(len(keep), dtype=torch.int64), torch.from_numpy(sizes)).to(device)
        b.series_ptr = series_ptr
        b.dom_ptr = dom_ptr
    elif isinstance(nd, IceMixNodes):
        # one sampling call over the whole batch: ptr / batch describe the kept rows, n_pulses stays the raw pulses
        nodes, node_ptr, ids = nd.sample_batch(x, torch.from_numpy(ptr).to(torch.int32).to(x.device))
        b = Batch(x=nodes.type(self.dtype))
        b.ptr = node_ptr.to(torch.int64)
        b.n_pulses = n_pulses.to(device)
        b.batch = torch.repeat_interleave(torch.arange(len(keep), dtype=torch.int64, device=b.ptr.device),
                                          b.ptr[1:] - b.ptr[:-1], output_size=int(nodes.shape[0]))
        b.pulse_ids = ids
    else:
        raise NotImplementedError(f"graphnet_amd: batch_from_raw builds NodesAsPulses, PercentileClusters, "
                                  f"NodeAsDOMTimeSeries and IceMixNodes nodes, not {nd.__class__.__name__}; use the "
                                  "per-event path")
    ed = self._edge_definition
    if ed is not None and hasattr(ed, "_nb_nearest_neighbours"):
        b.knn_k = int(ed._nb_nearest_neighbours)
        b.knn_columns = list(ed._columns)
    elif isinstance(ed, (MinkowskiKNNEdges, RadialEdges)):
        ed._record(b)
    for k, vals in (truth or {}).items():
        b[k] = torch.as_tensor(np.asarray([vals[i] for i in keep])).to(device)
    b["graph_definition"] = self.__class__.__name__
    return b


GraphDefinition.batch_from_raw = _batch_from_raw


class KNNGraph(GraphDefinition):
    """Edges drawn to the k nearest neighbours (``graphs/graphs.py:13-58``)."""

    def __init__(
        self,
        detector: Detector,
        node_definition: NodeDefinition = None,
        input_feature_names: Optional[List[str]] = None,
        dtype: Optional[torch.dtype] = torch.float,
        perturbation_dict: Optional[Dict[str, float]] = None,
        seed: Optional[Union[int, Generator]] = None,
        nb_nearest_neighbours: int = 8,
        columns: List[int] = [0, 1, 2],
        **kwargs: Any,
    ) -> None:
        super().__init__(
            detector=detector,
            node_definition=node_definition or NodesAsPulses(),
            edge_definition=KNNEdges(nb_nearest_neighbours=nb_nearest_neighbours, columns=columns),
            dtype=dtype,
            input_feature_names=input_feature_names,
            perturbation_dict=perturbation_dict,
            seed=seed,
            **kwargs,
        )
