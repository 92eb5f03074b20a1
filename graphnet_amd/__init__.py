"""graphnet_amd — MI355X-native DynEdge message-passing path behind graphnet's plugin API.

Host-side mirrors of the reference interface (``Data``/``Batch``, ``Detector``, ``KNNGraph``,
``GNN``/``DynEdge``, ``StandardModel``, tasks, losses) sit on top of a C-ABI shared library of
hand-written gfx950 HIP kernels (``include/graphnet_amd.h``).  Importing the package never
needs a GPU; calling a device op without the built library raises ``RuntimeError``.
"""
from .data import Batch, Data, collate_fn, collator_sequence_buckleting  # noqa: F401
from .detector import (  # noqa: F401
    Detector, IceCube86, IceCubeDeepCore, IceCubeKaggle, IceCubeUpgrade, ORCA150SuperDense, Prometheus,
)
from .model import Model, ModelConfig  # noqa: F401
from .graphs import (  # noqa: F401
    GraphDefinition, IceMixNodes, KNNEdges, KNNGraph, MinkowskiKNNEdges, NodeAsDOMTimeSeries, NodesAsPulses, PercentileClusters,
    RadialEdges,
)
from .gnn import GNN, DynEdge, DynEdgeConv, DynEdgeJINST  # noqa: F401
from .tito import DynEdgeTITO, DynTrans  # noqa: F401
from .rnn import Node_RNN, RNN_TITO  # noqa: F401
from .particlenet import ParticleNeT  # noqa: F401
from .icemix import (  # noqa: F401
    Attention_rel, Block, Block_rel, DeepIce, DropPath, FourierEncoder, Mlp, SinusoidalPosEmb, SpacetimeEncoder,
)
from .standard_model import (  # noqa: F401
    BinaryClassificationTask, BinaryClassificationTaskLogits, BinaryCrossEntropyLoss, DirectionReconstructionWithKappa,
    EnergyReconstruction, IdentityTask, LogCoshLoss, LossFunction, MSELoss, PiecewiseLinearLR,
    StandardLearnedTask, StandardModel, Task, VonMisesFisher2DLoss, VonMisesFisher3DLoss, VonMisesFisherLoss,
    ZenithReconstruction, ZenithReconstructionWithKappa,
)

__version__ = "0.1.0"
