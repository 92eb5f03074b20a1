"""``Node_RNN`` and ``RNN_TITO``: a GRU over every DOM's pulse series in front of ``DynEdgeTITO``.

Mirror of ``models/rnn/node_rnn.py`` and ``models/gnn/RNN_tito.py``.  The reference splits the batch into ~10^5 tensors,
packs them and calls ``torch.nn.GRU``; here the ragged recurrence is one kernel forward and one backward
(``gn_gru_series_fwd`` / ``gn_gru_series_bwd``, ``csrc/rnn.hip``), fp32 in both compute modes.  There is no torch fallback:
outside the kernels' envelope (``gn_gru_supported``) the forward raises.
"""
from __future__ import annotations

from typing import Any, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ops
from .data import Batch, Data
from .gnn import GNN, _maybe
from .tito import DynEdgeTITO


class _GRUSeriesFunction(torch.autograd.Function):
    """``out[M, H]``: final GRU state of every series; gradients for the four layer-0 tensors, none for ``xs``."""

    @staticmethod
    def forward(ctx, xs: Tensor, series_ptr: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor) -> Tensor:  # type: ignore[override]
        need = any(ctx.needs_input_grad[2:])
        out, saved = ops.gru_series_fwd(xs, series_ptr, w_ih, w_hh, b_ih, b_hh, save=need)
        if need:
            ctx.save_for_backward(xs, series_ptr, w_hh, saved)
        return out

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        xs, series_ptr, w_hh, saved = ctx.saved_tensors
        dw_ih, db_ih, dw_hh, db_hh = ops.gru_series_bwd(gout.to(torch.float32), saved, xs, series_ptr, w_hh)
        return None, None, dw_ih.contiguous(), dw_hh, db_ih, db_hh


def sinusoidal_pos_emb(x: Tensor, dim: int, n_freq: float = 10000.0) -> Tensor:
    """``SinusoidalPosEmb(dim)(x)`` of ``components/embedding.py:42-50`` (unscaled), the same fp32 operations in the same
    order: ``[..., dim]`` appended to the shape of ``x``.  The ``dim / 2`` frequencies are formed on the host and copied: the
    arguments reach ~10^4 rad, where one ulp of a frequency is 10^-3 rad, so the table must not depend on which ``exp`` a
    device has."""
    half_dim = dim / 2
    emb = torch.log(torch.tensor([n_freq], dtype=torch.float32)) / half_dim
    emb = torch.exp(torch.arange(half_dim) * (-emb)).to(x.device)
    emb = x.unsqueeze(-1) * emb.unsqueeze(0)
    return torch.cat((torch.sin(emb), torch.cos(emb)), dim=-1)


class Node_RNN(GNN):
    """One GRU state per DOM from its pulse series, joined to the DOM's summary features (``models/rnn/node_rnn.py``;
    constructor arguments, their order and defaults are the reference's; ``nb_outputs = hidden_size + 5``).

    Input: a device batch of :class:`~graphnet_amd.graphs.NodeAsDOMTimeSeries` rows, last column ``new_node_col``; the
    ``series_ptr`` / ``dom_ptr`` that ``batch_from_raw`` attaches are used when present, otherwise they are derived on the
    device from ``new_node_col`` and ``batch`` (one read-back of the series count).  Output: a batch with one row per DOM,
    ``x = [first row of the series without new_node_col, charge column = asinh(sum of the series' charges) | rnn_out]``,
    ``batch`` / ``ptr`` per DOM, ``n_pulses`` unchanged and no ``edge_index``: the k-NN on ``features_subset`` that the
    reference builds here (``node_rnn.py:130-134``) is the device k-NN of the backbone that follows
    (``DynEdgeTITO.set_backend(graph_columns=features_subset)``, ``compat`` mode), which computes the same graph.

    **Layer 0 only.**  The reference returns ``self._rnn(packed)[-1][0]`` (``node_rnn.py:111``): ``h_n[0]``, the final
    state of LAYER 0.  Layers ``k >= 1`` and the dropout between layers never reach its output.  This class therefore
    computes layer 0 alone; ``_rnn`` is a ``torch.nn.GRU`` that is never called and only holds the parameters under the
    reference's names (``_rnn.weight_ih_l{k}`` ... for every ``k < num_layers``), so that its checkpoints load.  The
    parameters of layers ``k >= 1`` get no gradient (``.grad`` stays ``None``), as in the reference.

    No gradient flows through the summed charge (in the reference it is a fresh ``torch.tensor``) nor into ``x``.
    """

    def __init__(self, nb_inputs: int, hidden_size: int, num_layers: int, time_series_columns: List[int],
                 nb_neighbours: int = 8, features_subset: Optional[List[int]] = None, dropout: float = 0.5,
                 embedding_dim: int = 0) -> None:
        self._hidden_size = hidden_size
        self._num_layers = num_layers
        self._time_series_columns = list(time_series_columns)
        self._nb_neighbors = nb_neighbours
        self._features_subset = features_subset
        self._embedding_dim = embedding_dim
        self._nb_inputs = nb_inputs
        super().__init__(nb_inputs, hidden_size + 5)
        if self._embedding_dim != 0:
            if self._embedding_dim % 2 != 0:
                raise ValueError(f"dim has to be even. Got: {self._embedding_dim}")
            self._nb_inputs = self._embedding_dim * nb_inputs
        # parameter container only (see the class docstring): forward() never calls it
        self._rnn = torch.nn.GRU(num_layers=self._num_layers, input_size=self._nb_inputs, hidden_size=self._hidden_size,
                                 batch_first=True, dropout=dropout)

    def clean_up_data_object(self, data: Any) -> Any:
        """Feature names of the output rows (``node_rnn.py:75-89``), where the batch carries names."""
        feats = _maybe(data, "features")
        if isinstance(feats, list) and feats and isinstance(feats[0], list):
            new = feats[0][:-1] + ["rnn_out_" + str(i) for i in range(self._hidden_size)]
            data.features = [new] * len(feats)
        return data

    def forward(self, data: Any) -> Batch:
        x = data.x
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.Node_RNN runs on an MI355X (HIP) device only; move the batch to 'cuda'.")
        if not ops.gru_supported(self._nb_inputs, self._hidden_size):
            raise RuntimeError(f"graphnet_amd.Node_RNN: GRU input size {self._nb_inputs} / hidden size {self._hidden_size} is "
                               "outside the kernels' envelope (gn_gru_supported: 1 <= I <= 32, 4 <= H <= 64, H % 4 == 0); "
                               "there is no torch fallback")
        x = x.to(torch.float32)
        N, F = int(x.shape[0]), int(x.shape[1]) - 1
        n_events = int(data.n_pulses.shape[0])
        series_ptr, dom_ptr = _maybe(data, "series_ptr"), _maybe(data, "dom_ptr")
        if series_ptr is None or dom_ptr is None:
            heads = torch.nonzero(x[:, -1]).flatten()
            series_ptr = torch.cat([heads, torch.tensor([N], dtype=heads.dtype, device=x.device)]).to(torch.int32)
            dom_ptr = torch.zeros(n_events + 1, dtype=torch.int32, device=x.device)
            dom_ptr[1:] = torch.cumsum(torch.bincount(data.batch[heads].to(torch.int64), minlength=n_events), 0)
        series_ptr, dom_ptr = series_ptr.to(torch.int32), dom_ptr.to(torch.int32)
        M = int(series_ptr.shape[0]) - 1
        time_series = x[:, self._time_series_columns]
        if self._embedding_dim != 0:
            time_series = sinusoidal_pos_emb(time_series * 4096, self._embedding_dim).reshape(
                (N, self._embedding_dim * len(self._time_series_columns)))
        time_series = time_series.contiguous()
        if int(time_series.shape[1]) != self._nb_inputs:
            raise ValueError(f"Node_RNN: {len(self._time_series_columns)} time series columns do not give the GRU's "
                             f"{self._nb_inputs} inputs")
        g = self._rnn
        rnn_out = _GRUSeriesFunction.apply(time_series.detach(), series_ptr, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0,
                                           g.bias_hh_l0)
        dom = ops.dom_series_summary(x, series_ptr, F, self._time_series_columns[0])
        out = Batch()
        if isinstance(data, Data):
            for k, v in data.items():
                if k not in ("x", "edge_index", "nbr_table", "series_ptr", "dom_ptr", "batch", "ptr"):
                    out[k] = v
        else:
            out.n_pulses = data.n_pulses
        out.x = torch.cat([dom, rnn_out], dim=1)
        out.ptr = dom_ptr.to(torch.int64)
        out.batch = ops.ptr_to_batch(dom_ptr, M).to(torch.int64)
        return self.clean_up_data_object(out)


class RNN_TITO(GNN):
    """``Node_RNN`` followed by ``DynEdgeTITO`` (``models/gnn/RNN_tito.py``; constructor arguments, their order and defaults
    are the reference's), for data with many pulses per DOM.  Sub-modules ``_rnn`` and ``_dynedge_tito`` carry the
    reference's state-dict keys.  Takes the batches of a graph definition with
    :class:`~graphnet_amd.graphs.NodeAsDOMTimeSeries` nodes.

    ``embedding_dim=None`` (the default) means no embedding, as the reference's docstring says.  The reference itself
    raises a ``TypeError`` there (``Node_RNN`` computes ``None * nb_inputs``); here ``None`` is taken as 0.
    """

    def __init__(self, nb_inputs: int, time_series_columns: List[int], *, nb_neighbours: int = 8, rnn_layers: int = 2,
                 rnn_hidden_size: int = 64, rnn_dropout: float = 0.5, features_subset: Optional[List[int]] = None,
                 dyntrans_layer_sizes: Optional[List[Tuple[int, ...]]] = None,
                 post_processing_layer_sizes: Optional[List[int]] = None, readout_layer_sizes: Optional[List[int]] = None,
                 global_pooling_schemes: List[str] = ["max"], embedding_dim: Optional[int] = None, n_head: int = 16,
                 use_global_features: bool = True, use_post_processing_layers: bool = True):
        self._nb_neighbours = nb_neighbours
        self._nb_inputs = nb_inputs
        self._rnn_layers = rnn_layers
        self._rnn_hidden_size = rnn_hidden_size
        self._rnn_dropout = rnn_dropout
        self._embedding_dim = embedding_dim
        self._n_head = n_head
        self._use_global_features = use_global_features
        self._use_post_processing_layers = use_post_processing_layers
        self._features_subset = features_subset
        if dyntrans_layer_sizes is None:
            dyntrans_layer_sizes = [(256, 256)] * 4
        else:
            dyntrans_layer_sizes = [tuple(layer_sizes) for layer_sizes in dyntrans_layer_sizes]
        self._dyntrans_layer_sizes = dyntrans_layer_sizes
        self._post_processing_layer_sizes = post_processing_layer_sizes
        self._global_pooling_schemes = global_pooling_schemes
        if readout_layer_sizes is None:
            readout_layer_sizes = [256, 128]
        self._readout_layer_sizes = readout_layer_sizes
        super().__init__(nb_inputs, self._readout_layer_sizes[-1])
        self._rnn = Node_RNN(nb_inputs=2, hidden_size=self._rnn_hidden_size, num_layers=self._rnn_layers,
                             time_series_columns=time_series_columns, nb_neighbours=self._nb_neighbours,
                             features_subset=self._features_subset, dropout=self._rnn_dropout,
                             embedding_dim=0 if self._embedding_dim is None else self._embedding_dim)
        self._dynedge_tito = DynEdgeTITO(
            nb_inputs=self._rnn_hidden_size + 5, dyntrans_layer_sizes=self._dyntrans_layer_sizes,
            features_subset=self._features_subset, global_pooling_schemes=self._global_pooling_schemes,
            use_global_features=self._use_global_features, use_post_processing_layers=self._use_post_processing_layers,
            post_processing_layer_sizes=self._post_processing_layer_sizes, readout_layer_sizes=self._readout_layer_sizes,
            n_head=self._n_head, nb_neighbours=self._nb_neighbours)
        self.set_backend()

    def set_backend(self, *, dtype: str = "bf16", knn_mode: str = "compat",
                    graph_columns: Optional[Sequence[int]] = None) -> "RNN_TITO":
        """Passed through to ``DynEdgeTITO.set_backend`` (the GRU is fp32 in both modes).  ``graph_columns`` defaults to
        ``features_subset``: the columns of the k-NN that ``Node_RNN`` rebuilds in the reference."""
        if graph_columns is None:
            graph_columns = self._features_subset or [0, 1, 2, 3]
        self._dynedge_tito.set_backend(dtype=dtype, knn_mode=knn_mode, graph_columns=graph_columns)
        return self

    def forward(self, data: Any, return_trace: bool = False) -> Tensor:
        data = self._rnn(data)
        return self._dynedge_tito(data, return_trace=return_trace) if return_trace else self._dynedge_tito(data)
