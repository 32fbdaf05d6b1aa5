"""hgnn on MI355X: the hetero SAGE message-passing hot path of ramkp990/Truth_Recommendation_GNN,
rebuilt as hand-written gfx950 HIP kernels behind a C ABI (``include/hgnn.h``), with the
reference's PyG-style Python surface (``SAGEConv``, ``HeteroData``, ``WeightedRGCN``).

fp32 throughout by default.  ``HGNN_ROW_DTYPE=bf16`` (read at import into ``ops.ROW_DTYPE``), or
``row_dtype="bf16"`` on the models, ``ops.LayerSpec`` and ``ops.edge_bce_loss``, stores the rows
the forward gathers and the link loss read per edge as bf16 (``ops.rows_to_bf16``); everything
else stays fp32.  ``HGNN_GRAD_ROW_DTYPE=bf16`` (``ops.GRAD_ROW_DTYPE``; ``grad_row_dtype="bf16"``
on the models and ``ops.LayerSpec``) is a second, independent opt-in: the backward's K2 scatters
read bf16 copies of their gradient tables.  ``evaluate`` / ``recommend`` take their own ``row_dtype`` (default "fp32") or
bf16 tables, and then rank the rows rounded to bf16 on bf16 MFMA.
"""
from .graph import HeteroData, RelationCSR, relation_csr, CSR_CACHE  # noqa: F401
from .nn import SAGEConv, WeightedRGCN, WeightedRGCNAuthor, HeteroSAGE  # noqa: F401
from . import ops, synth  # noqa: F401
from .ops import PostDistribution, SkewedNegatives, mine_hard_negatives  # noqa: F401
from .ops import (edge_bce_loss, edge_softmax_loss, edge_softmax_loss_raw,  # noqa: F401
                  link_softmax_loss)
from .metrics import SeenIndex, evaluate, recommend  # noqa: F401

__version__ = "0.1.0"
