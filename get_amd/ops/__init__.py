"""Autograd-aware host wrappers over the C-ABI (one ``torch.autograd.Function`` per fused op), one module per family.

PyTorch supplies device memory, streams and the autograd tape; every numerical
step runs in libget_hip.so.  All tensors are fp32/contiguous on a ROCm device.

This file only re-exports the public names: callers look an op up on the package at call time (`ops.att_flow(...)`),
so a tool may swap one by assignment.  Private helpers and the three mutable flags of `streams` stay in their modules.
"""
from . import _util, attention, bert, bidaf, dense, embed, graph, loss, match, optim, pair, rank, rnn, streams, weights  # noqa: F401
from .attention import add_layernorm, concat_att, mha_sdpa, query_att, tanh_att  # noqa: F401
from .bert import bert_attention, bert_embed, gelu, tanh_act  # noqa: F401
from .bidaf import att_flow, highway  # noqa: F401
from .dense import (CLS_EXTRA, Segments, adam_step_flat, backward, cls_metrics, cross_entropy, evd_assemble, linear,  # noqa: F401
                    linear_wgrad_bf16, masked_mean, seg_broadcast, seg_pad)
from .embed import EMBED_CHUNK, embed_plan, embedding, embedding_backward  # noqa: F401
from .graph import (GAT_ELU, GAT_OUTPUT, GAT_PLAIN, GCNAdj, PackedAdj, RaggedPlan, as_packed, bf16_cell_ok,  # noqa: F401
                    dropout_mask_reference, feat_dropout, fused_dropout_ok, gat_dropout_mask, gat_layer, gat_pattern, gcn_scale,
                    ggnn_cell, graph_build, gsl_topk, new_dropout_seed, relu, scorer_fusable, scorer_gsl, spmm)
from .loss import softmax_cross_entropy  # noqa: F401
from .match import LIN_ATT_MODES, MATCH_BCAST_OPS, gauss_kernel, lin_att, match_bcast, match_dot, soft_align  # noqa: F401
from .optim import (FlatAdamW, SegmentTable, adamw_block_map, adamw_segment, adamw_segment_table, adamw_step_flat,  # noqa: F401
                    grad_norm_flat, grad_norm_partials)
from .rank import rank_cross_entropy, rank_hinge, rank_metrics  # noqa: F401
from .rnn import gru_seq, lstm_seq  # noqa: F401
from .streams import pending_side_stream, side_join, side_mark_backward, side_stream  # noqa: F401
from .weights import bf16_twins, bump_weight_epoch, derived, fp32x3p_guard, refresh_transposes, transposed  # noqa: F401
