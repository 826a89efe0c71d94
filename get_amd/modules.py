"""Drop-in ``nn.Module`` mirror of the reference's hot-path classes, backed by libget_hip.so.

Same class names, constructor arguments, ``forward()`` signatures, parameter names and shapes
as upstream, so ``MasterFC/master_get.py`` and reference checkpoints
load unchanged:

  Models/BiDAF/wrapper.py                      Linear, GGNN, GSL, GGNN_with_GSL, LSTM, GRU,
                                               GraphAttentionLayer, GAT, GCN
  thirdparty/two_branches_attention.py         ConcatNotEqualSelfAtt, ConcatSelfAtt, Dot, BiLinear, BiLinearTanh,
                                               ScaledDotProductAttention, MultiHeadAttentionOriginal,
                                               ConcatNotEqualSelfAttTransFormer, MultiHeadAttentionSimple, CoDaAttention
  thirdparty/self_attention.py                 MultiHeadSelfAttentionICLR2017Extend, SelfAttentionICLR2017,
                                               MultiHeadSelfAttentionICLR17OnWord, SelfAttentionType
  Models/FCWithEvidences/graph_based_semantic_structure.py   Graph_basedSemantiStructure
  Models/BiDAF/bidaf_model.py                  BiDAF
  matchzoo/modules                             Attention, BidirectionalAttention, MatchModule, Matching, GaussianKernel,
                                               RNNDropout, StackedBRNN, BertModule (get_amd/bert.py, re-exported here)
  matchzoo/losses                              RankHingeLoss, RankCrossEntropyLoss

(The tensor math outside the reference's modules -- the interaction helpers of torch_utils.py, layers.MovingAverage and the
matching histogram -- is in get_amd/pairwise.py.)

Adjacency arguments may be the reference's dense ``(N,R,R)`` tensors (any float dtype; packed once
on the device, values kept exactly) or a native :class:`get_amd.ops.PackedAdj` from
:func:`get_amd.ops.graph_build`.
"""
from __future__ import annotations

from enum import IntEnum
from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .keywords import KeyWordSettings
from .ops import PackedAdj


def _drop_caches_on_load(module: nn.Module):
    """The forward reads cached derivatives of the weights (transposes, fused bias sums, packed scalar gates; ops.transposed
    / ops.derived) that are validated by tensor identity and in-place version.  load_state_dict copies
    into the parameters in place; every module here drops ALL cached derivatives after a load so that no stale entry can
    survive whatever the copy path did to the version counters.  Any OTHER raw `.data` write (EMA swaps, hand-written
    optimisers) must call ops.bump_weight_epoch() itself (it clears every derived entry, frozen ones included)."""
    module.register_load_state_dict_post_hook(lambda m, incompatible_keys: ops.bump_weight_epoch())


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:330-347
class Linear(nn.Module):
    def __init__(self, in_features, out_features, bias=True, dropout=0.0):
        super().__init__()
        _drop_caches_on_load(self)
        self.linear = nn.Linear(in_features=in_features, out_features=out_features, bias=bias)
        if dropout > 0:
            self.dropout = nn.Dropout(p=dropout)
        self.reset_params()

    def reset_params(self):
        # kaiming-normal weights; the reference's bias-zeroing branch never fires (wrapper.py:341),
        # so biases keep nn.Linear's default init
        nn.init.kaiming_normal_(self.linear.weight)

    def forward(self, x):
        if hasattr(self, "dropout"):
            x = self.dropout(x)
        return ops.linear(x, self.linear.weight, self.linear.bias)


# ------------------------------------------------------------------ Models/base_model.py:144-162 (the layers it builds)
class Embedding(nn.Embedding):
    """torch.nn.Embedding whose GPU lookup and table gradient run in the library (ops.embedding): same constructor and
    ``from_pretrained``, the single state_dict key ``weight``, ``padding_idx`` honoured (its row receives no gradient).  The
    gradient of a trainable table is a row sum in a fixed order -- two backward passes give the same bits, which
    index_add_ / ATen's atomics do not promise -- and lands straight in ``weight.grad`` under a dist.FlatTrainer.
    ``max_norm``, ``scale_grad_by_freq`` and ``sparse=True`` are refused at construction: the reference sets none of them.
    A CPU weight takes torch's own forward (the models are constructed, loaded and inspected on the CPU)."""

    def __init__(self, num_embeddings, embedding_dim, padding_idx=None, max_norm=None, norm_type=2.0, scale_grad_by_freq=False,
                 sparse=False, **kwargs):
        if max_norm is not None or scale_grad_by_freq or sparse:
            raise ValueError("get_amd.modules.Embedding: max_norm, scale_grad_by_freq and sparse=True are not supported "
                             "(torch.nn.Embedding has them)")
        super().__init__(num_embeddings, embedding_dim, padding_idx=padding_idx, max_norm=None, norm_type=norm_type,
                         scale_grad_by_freq=False, sparse=False, **kwargs)

    def forward(self, input):
        if not self.weight.is_cuda:
            return super().forward(input)
        return ops.embedding(self.weight, input, self.padding_idx)


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:174-208
class GGNN(nn.Module):
    def __init__(self, in_features, out_features, dropout=0.2):
        super().__init__()
        self.proj = Linear(in_features, out_features, bias=False)
        self.linearz0 = Linear(out_features, out_features)
        self.linearz1 = Linear(out_features, out_features)
        self.linearr0 = Linear(out_features, out_features)
        self.linearr1 = Linear(out_features, out_features)
        self.linearh0 = Linear(out_features, out_features)
        self.linearh1 = Linear(out_features, out_features)
        if dropout > 0:
            self.dropout = nn.Dropout(p=dropout)

    def _params(self):
        g = lambda m: (m.linear.weight, m.linear.bias)
        return (self.proj.linear.weight, *g(self.linearz0), *g(self.linearz1), *g(self.linearr0), *g(self.linearr1),
                *g(self.linearh0), *g(self.linearh1))

    def _drop(self):
        """(p, seed) of the fused input dropout for this call, or None to use the materialised nn.Dropout."""
        if not (hasattr(self, "dropout") and self.training and self.dropout.p > 0):
            return (0.0, 0)
        w = self.proj.linear.weight
        if ops.fused_dropout_ok(w.shape[1], w.shape[0]):
            return (float(self.dropout.p), ops.new_dropout_seed())
        return None

    def forward(self, adj, x, plan=None, rows=0, score=None):
        """adj: dense (N,R,R) or PackedAdj; x: (N,R,Din).  Returns (N,R,Dout).
        Training-mode input dropout (wrapper.py:189-190) runs inside the first GEMM's loader.
        plan (ops.RaggedPlan, internal fast path): x is node-compact (>= rows, Din); returns (rows, Dout).
        score (internal, see ops.ggnn_cell): also return the consuming word scorer's projection of the output."""
        adj = ops.as_packed(adj)
        d = self._drop()
        if d is None:
            return ops.ggnn_cell(adj, self.dropout(x), None, self._params(), plan=plan, rows=rows, score=score)
        return ops.ggnn_cell(adj, x, None, self._params(), d[0], d[1], plan=plan, rows=rows, score=score)

    def forward_ids(self, adj, embedding: nn.Embedding, ids: torch.Tensor, plan=None, rows=0, score=None):
        """Same cell on ``embedding(ids)`` with the row gather fused into the first GEMM
        (graph_based_semantic_structure.py:100,150); training-mode dropout is applied there too.  Falls
        back to an explicit lookup + nn.Dropout only for widths that are not float4-shaped.
        plan: node-compact layout, the ids come from ``plan.cids``; returns (rows, Dout)."""
        adj = ops.as_packed(adj)
        d = self._drop()
        if plan is not None:
            rows = rows or plan.m_real
            ids = plan.cids[:rows]
        if d is None:
            x = self.dropout(embedding(ids.long()))
            return ops.ggnn_cell(adj, x, None, self._params(), plan=plan, rows=rows, score=score)
        return ops.ggnn_cell(adj, embedding.weight, ids.to(torch.int32).reshape(-1), self._params(), d[0], d[1],
                             plan=plan, rows=rows, score=score)


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:210-227
class GSL(nn.Module):
    def __init__(self, rate):
        super().__init__()
        self.rate = rate

    def forward(self, adj, score):
        """Keep the top int(rate*N) nodes' rows and columns (union), no renormalisation, no gradient.
        Dense adjacency in -> dense refined adjacency out; PackedAdj in -> PackedAdj with keep-set."""
        n_nodes = adj.r if isinstance(adj, PackedAdj) else adj.shape[-1]
        k = int(self.rate * n_nodes)
        keep = ops.gsl_topk(score.reshape(score.shape[0], n_nodes), k)
        if isinstance(adj, PackedAdj):
            return adj.with_keep(keep)
        return PackedAdj.from_dense(adj).with_keep(keep).to_dense().to(adj.dtype)


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:153-172
class GGNN_with_GSL(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, rate=0.8, dropout=0.2):
        super().__init__()
        self.feat_prop1 = GGNN(input_dim, hidden_dim, dropout)
        self.word_scorer1 = GGNN(hidden_dim, 1, dropout)
        self.gsl1 = GSL(rate)
        self.feat_prop2 = GGNN(hidden_dim, output_dim, dropout)
        self.last_score = None     # observables of the last forward (scores, keep words) for analysis/tests
        self.last_keep = None
        # called (no arguments) during backward as soon as the gradient w.r.t. the first cell's output exists: from
        # then on only the first cell's own gradients are still to come (dist.FlatTrainer.attach_overlap)
        self.grad_milestone_hook = None

    def _milestone(self, feat):
        hook = self.grad_milestone_hook
        if hook is not None and feat.requires_grad:
            def fire(g, _hook=hook):
                _hook()
                return g
            feat.register_hook(fire)

    def _gate12(self):
        s = self.word_scorer1
        srcs = []
        for m in (s.linearz0, s.linearz1, s.linearr0, s.linearr1, s.linearh0, s.linearh1):
            srcs += [m.linear.weight, m.linear.bias]
        # the scorer's parameters never receive a gradient (wrapper.py:219: no gradient through top-k), so a FlatTrainer
        # leaves them out of its bucket and never rewrites them: the packed copy then only depends on tensor identity /
        # in-place version, not on the optimiser's weight epoch (one cat launch + a dozen host ops less per step)
        static = not any(getattr(t, "_gh_direct_grad", False) for t in srcs)
        return ops.derived("gate12", tuple(srcs), lambda: torch.cat([t.detach().reshape(1) for t in srcs]), frozen=static)

    def _scorer_drop(self):
        """(p, seed) of word_scorer1's own input dropout for this call (wrapper.py:189-190)."""
        s = self.word_scorer1
        if hasattr(s, "dropout") and self.training and s.dropout.p > 0:
            return float(s.dropout.p), ops.new_dropout_seed()
        return 0.0, 0

    def _score_arg(self):
        """Argument that makes the first cell's last epilogue also produce the scorer's projection (or None)."""
        w = self.word_scorer1.proj.linear.weight
        if not ops.scorer_fusable(w.shape[1]):
            return None
        return (w,) + self._scorer_drop()

    def _refine(self, adj: PackedAdj, feat, plan=None, collapsed=False, score_x=None):
        s = self.word_scorer1
        drop_p, seed = (0.0, 0) if score_x is not None else self._scorer_drop()
        k = int(self.gsl1.rate * adj.r)
        score, keep = ops.scorer_gsl(adj, feat, s.proj.linear.weight, self._gate12(), k, drop_p, seed, plan=plan,
                                     collapsed=collapsed, score_x=score_x)
        self.last_score, self.last_keep = score, keep
        return adj.with_keep(keep)

    def _first_cell(self, run):
        """Run feat_prop1 through `run(score)`; returns (feat, score_x or None)."""
        sc = self._score_arg()
        res = run(sc)
        return res if sc is not None else (res, None)

    def forward(self, adj, feat):
        adj = ops.as_packed(adj)
        feat, sx = self._first_cell(lambda sc: self.feat_prop1(adj, feat, score=sc))
        self._milestone(feat)
        adj_refined = self._refine(adj, feat, score_x=sx)
        return self.feat_prop2(adj_refined, feat)

    def forward_ids(self, adj, embedding, ids, plan=None):
        """plan (ops.RaggedPlan): node-compact fast path -- the first cell and the scorer run on every row (the
        padding nodes' scores compete in the top-k), the second cell on the real-node rows only; returns
        (plan.m_real, H) instead of (N,R,H)."""
        adj = ops.as_packed(adj)
        if plan is None:
            feat, sx = self._first_cell(lambda sc: self.feat_prop1.forward_ids(adj, embedding, ids, score=sc))
            self._milestone(feat)
            adj_refined = self._refine(adj, feat, score_x=sx)
            return self.feat_prop2(adj_refined, feat)
        # without dropout (evaluation) every padding row of the batch is the same vector: the first cell then runs on
        # the real rows plus ONE representative padding row instead of all n*R rows
        collapsed = not self.training
        rows = min(plan.m_real + 1, plan.m_tot) if collapsed else plan.m_tot
        feat, sx = self._first_cell(lambda sc: self.feat_prop1.forward_ids(adj, embedding, ids, plan=plan, rows=rows, score=sc))
        self._milestone(feat)
        adj_refined = self._refine(adj, feat, plan, collapsed, score_x=sx)
        return self.feat_prop2(adj_refined, feat, plan=plan, rows=plan.m_real)


class _SeqEncoder(nn.Module):
    """What the LSTM and GRU drop-ins share: ``self.rnn`` (torch's module of ``_rnn_class``, a holder of parameters only), the
    reference's init of one layer and direction, and the layer loop of forward around the cell's own ``_layer``."""
    _rnn_class = None

    def __init__(self, input_size, hidden_size, batch_first, num_layers, bidirectional, dropout, reset_params=True):
        super().__init__()
        _drop_caches_on_load(self)
        self.rnn = self._rnn_class(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers,
                                   bidirectional=bidirectional, batch_first=batch_first)
        if reset_params:
            self.reset_params()
        self.dropout = nn.Dropout(p=dropout)
        self.last_seed = None       # input-dropout seed of the last training-mode forward (ops.feat_dropout)

    def _suffixes(self):
        return ("", "_reverse") if self.rnn.bidirectional else ("",)

    def _param(self, kind, i, sfx):
        return getattr(self.rnn, "%s_l%s%s" % (kind, i, sfx))

    def _reset_one(self, i, sfx):
        nn.init.orthogonal_(self._param("weight_hh", i, sfx))
        nn.init.kaiming_normal_(self._param("weight_ih", i, sfx))
        nn.init.constant_(self._param("bias_hh", i, sfx), val=0)
        nn.init.constant_(self._param("bias_ih", i, sfx), val=0)

    def reset_params(self):
        for i in range(self.rnn.num_layers):
            for sfx in self._suffixes():
                self._reset_one(i, sfx)

    def _layer(self, i, inp, lens, order, T):
        """Layer i on `inp`: the input projections of its directions and the cell's recurrence op.  Returns y and h_n."""
        raise NotImplementedError

    def forward(self, x, return_h=True, max_len=None):
        inp, lens, order, T, d_new_indices = _rnn_inputs(self, self._rnn_class.__name__, x, max_len)
        states = []
        for i in range(self.rnn.num_layers):
            inp, h_n = self._layer(i, inp, lens, order, T)
            states.append(h_n)
        return inp, _rnn_state(states, return_h, d_new_indices)


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:229-276
class LSTM(_SeqEncoder):
    """The reference's LSTM sequence encoder on the HIP recurrence kernels (ops.lstm_seq).  ``self.rnn`` only holds the
    parameters (state_dict keys ``rnn.weight_ih_l0`` ...): it is never called, neither MIOpen nor nn.LSTM.forward runs.

    forward((x, x_len, d_new_indices, d_restoring_indices), return_h=True, max_len=None):
      x (B,L,D) on the device; x_len (B,) any integer dtype on either device; the index pair must be inverse permutations
      (as the reference requires); d_new_indices -- the reference's order by descending length -- only sets the order in
      which sequences are tiled, the outputs are in the rows of x.
      T = max_len when given (no host synchronisation then), else max(x_len) as in the reference -- one read-back when
      x_len lives on the device.  A CPU x_len with a length < 1 or > T raises ValueError as the reference's pack / pad
      functions do; a device x_len is clamped into [0, min(L, T)] by the kernel instead, and a length of 0 gives zero rows
      and a zero final state (pack_padded_sequence raises there).
      Returns y (B,T,dirs*H), zero at t >= len, and h: (B, layers*dirs*H) in the rows of x when return_h, else the raw
      (layers*dirs, B, H) tensor in the sorted order, as the reference returns it.
    Training mode: input dropout with the stateless mask of ops.feat_dropout, its seed kept in ``last_seed``.  There is no
    dropout between layers (the reference passes none to nn.LSTM).  ``batch_first`` is accepted and irrelevant, as in the
    reference, whose forward hard-codes batch-first packing."""

    _rnn_class = nn.LSTM

    def __init__(self, input_size, hidden_size, batch_first=False, num_layers=1, bidirectional=False, dropout=0.2,
                 _reset_params=True):
        # (Graph_basedSemantiStructure keeps nn.LSTM's own init: its seeded construction must not move)
        super().__init__(input_size, hidden_size, batch_first, num_layers, bidirectional, dropout, _reset_params)

    def _layer(self, i, inp, lens, order, T):
        return _lstm_layer(lambda kind, sfx: self._param(kind, i, sfx), self._suffixes(), inp, lens, order, T)


def _lstm_layer(param, suffixes, inp, lens, order, T):
    """One LSTM layer on `inp` (B,L,D): the input projection of each direction (ops.linear, both biases folded into it) and the
    recurrence (ops.lstm_seq).  param(kind, suffix) gives the layer's parameters.  Returns y (B,T,dirs*H) and h_n."""
    gx, w_hh = [], []
    for sfx in suffixes:
        bias = param("bias_ih", sfx) + param("bias_hh", sfx)
        gx.append(ops.linear(inp, param("weight_ih", sfx), bias))
        w_hh.append(param("weight_hh", sfx))
    return ops.lstm_seq(gx, w_hh, lens, order, T)[:2]


def _gru_layer(param, suffixes, inp, lens, order, T):
    """One GRU layer on `inp`: as _lstm_layer, with b_hh staying with the recurrence (ops.gru_seq)."""
    gx, w_hh, b_hh = [], [], []
    for sfx in suffixes:
        gx.append(ops.linear(inp, param("weight_ih", sfx), param("bias_ih", sfx)))
        w_hh.append(param("weight_hh", sfx))
        b_hh.append(param("bias_hh", sfx))
    return ops.gru_seq(gx, w_hh, b_hh, lens, order, T)


def _rnn_inputs(module, who, x, max_len):
    """The argument handling LSTM.forward and GRU.forward share: the 4-tuple, T, the host-side length check, the device
    lengths and tiling order, the input dropout with its seed kept in ``module.last_seed``."""
    x, x_len, d_new_indices, d_restoring_indices = x
    assert x.dim() == 3, who + ": x is (B, L, D)"
    x_len = torch.as_tensor(x_len)
    assert x_len.shape == (x.shape[0],) and not x_len.dtype.is_floating_point, who + ": x_len is an integer (B,) tensor"
    if max_len is not None:
        T = int(max_len)
    else:
        T = int(x_len.max())        # (a device x_len is read back here; the model always passes max_len)
    if not x_len.is_cuda and (int(x_len.max()) > T or int(x_len.min()) < 1):
        raise ValueError("%s: every length must lie in [1, %d], got [%d, %d]" % (who, T, int(x_len.min()), int(x_len.max())))
    _lib.require_cuda(x)
    lens = x_len.to(device=x.device, dtype=torch.int32, non_blocking=True)
    order = torch.as_tensor(d_new_indices).to(device=x.device, dtype=torch.int32, non_blocking=True)
    p, seed = _encoder_drop(module.training, module.dropout.p)
    module.last_seed = seed if p > 0 else None
    return ops.feat_dropout(x, p, seed), lens, order, T, d_new_indices


def _rnn_state(states, return_h, d_new_indices):
    """The second value of the two encoders from the per-layer (dirs, B, H) final states: (B, layers*dirs*H) in the rows of x
    when return_h, else the raw (layers*dirs, B, H) tensor in the sorted order."""
    h = states[0] if len(states) == 1 else torch.cat(states, dim=0)
    if return_h:
        return h.permute(1, 0, 2).reshape(h.shape[1], -1)
    return h[:, torch.as_tensor(d_new_indices).to(h.device).long()]


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:279-327
class GRU(_SeqEncoder):
    """The reference's GRU sequence encoder on the HIP recurrence kernels (ops.gru_seq).  ``self.rnn`` only holds the
    parameters (state_dict keys ``rnn.weight_ih_l0`` ...): it is never called, neither MIOpen nor nn.GRU.forward runs.

    This is the reference's constructor with its one raising line made runnable: upstream's ``reset_params`` ends each layer and
    direction with ``bias_hh.chunk(4)[1].fill_(1)`` on a leaf parameter that requires grad, which raises, so upstream's class
    cannot be constructed as written.  Here the same statements run in the same order under ``torch.no_grad()`` -- the
    one-line repair a user of the reference makes.  ``chunk(4)`` of the 3H-vector gives pieces of ceil(3H/4) elements, so the
    ones land on elements [ceil(3H/4), 2 ceil(3H/4)): they straddle the r and z thirds (the tail of r, the head of z), not
    one gate as the LSTM-style forget-bias idiom intends.  That is kept exactly as written.

    forward((x, x_len, d_new_indices, d_restoring_indices), return_h=True, max_len=None): the contract of :class:`LSTM` --
    T, the host-side ValueError for lengths outside [1, T], device lengths clamped (a length of 0 gives zero rows and a zero
    state), d_new_indices used only as tiling order, outputs in the rows of x, y (B,T,dirs*H) zero at t >= len, h as there.
    Training mode: input dropout by ops.feat_dropout with its seed kept in ``last_seed``; no dropout between layers."""

    _rnn_class = nn.GRU

    def __init__(self, input_size, hidden_size, batch_first=False, num_layers=1, bidirectional=False, dropout=0.2):
        super().__init__(input_size, hidden_size, batch_first, num_layers, bidirectional, dropout)

    def _reset_one(self, i, sfx):
        # wrapper.py:291-304, statement by statement, under no_grad (the fill_ of a view of a leaf raises otherwise)
        with torch.no_grad():
            super()._reset_one(i, sfx)
            self._param("bias_hh", i, sfx).chunk(4)[1].fill_(1)

    def _layer(self, i, inp, lens, order, T):
        return _gru_layer(lambda kind, sfx: self._param(kind, i, sfx), self._suffixes(), inp, lens, order, T)


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:7-67
class GraphAttentionLayer(nn.Module):
    """One GAT head: h = input W, masked (adj > 0) LeakyReLU edge softmax, attention dropout, att @ h, elu if concat.
    A row without an edge attends uniformly to all L nodes (the reference's -9e15 fill).  W is (in, out), a (2 out, 1)."""

    def __init__(self, in_features, out_features, dropout, alpha, concat=True):
        super().__init__()
        _drop_caches_on_load(self)
        self.dropout = dropout
        self.in_features = in_features
        self.out_features = out_features
        self.alpha = alpha
        self.concat = concat
        self.W = nn.Parameter(torch.zeros(size=(in_features, out_features)))
        nn.init.xavier_uniform_(self.W.data, gain=1.414)
        self.a = nn.Parameter(torch.zeros(size=(2 * out_features, 1)))
        nn.init.xavier_uniform_(self.a.data, gain=1.414)
        self.leakyrelu = nn.LeakyReLU(self.alpha)
        self.last_seed = None       # attention-dropout seed of the last training-mode forward (ops.gat_dropout_mask)

    def forward(self, input, adj):
        """input (B,L,in); adj dense (B,L,L) or PackedAdj.  Returns (B,L,out)."""
        adj = ops.gat_pattern(adj)
        p, seed = _encoder_drop(self.training, self.dropout)
        self.last_seed = seed if p > 0 else None
        mode = ops.GAT_ELU if self.concat else ops.GAT_PLAIN
        return ops.gat_layer(input, adj, [self], mode, 0, p, seed)

    def __repr__(self):
        return self.__class__.__name__ + " (" + str(self.in_features) + " -> " + str(self.out_features) + ")"


def _encoder_drop(training: bool, p: float):
    """(p, seed) of a training-mode dropout of the encoders, (0.0, 0) otherwise."""
    if training and p > 0:
        return float(p), ops.new_dropout_seed()
    return 0.0, 0


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:70-112
class GAT(nn.Module):
    """Dense GAT of the reference on the packed adjacency: every layer's heads in one projection GEMM and one
    aggregation launch (ops.gat_layer).  Output: relu(sum of the output heads / L), L = x.size(1)."""

    def __init__(self, input_size, hidden_size, output_size, head_num=3, num_layers=1, dropout=0.6, alpha=0.2):
        super().__init__()
        _drop_caches_on_load(self)
        self.dropout = dropout
        self.attentions = []
        for _ in range(num_layers - 1):
            self.attentions.append([GraphAttentionLayer(input_size, hidden_size, dropout=dropout, alpha=alpha, concat=True)
                                    for _ in range(head_num)])
            input_size = hidden_size * head_num
        for i, layer in enumerate(self.attentions):
            for j, attention in enumerate(layer):
                self.add_module("layer_{}_{}".format(i, j), attention)
        self.out_att = nn.ModuleList([GraphAttentionLayer(input_size, output_size, dropout=dropout, alpha=alpha, concat=False)
                                      for _ in range(head_num)])
        # training mode: the seeds of the last forward, in order (input dropout, then per layer: attention dropout,
        # and the dropout in front of the output layer) -- ops.feat_dropout / ops.gat_dropout_mask replay them
        self.last_seeds = None

    def forward(self, x, adj):
        """x (B,L,input_size); adj dense (B,L,L) or PackedAdj.  Returns (B,L,output_size)."""
        adj = ops.gat_pattern(adj)
        assert x.size(1) == adj.r, "GAT: x.size(1) must be the adjacency's node count"
        seeds = []

        def drop():
            p, seed = _encoder_drop(self.training, self.dropout)
            seeds.append(seed)
            return p, seed

        x = ops.feat_dropout(x, *drop())
        for li, heads in enumerate(self.attentions):
            x = ops.gat_layer(x, adj, heads, ops.GAT_ELU, li, *drop())
        x = ops.feat_dropout(x, *drop())
        x = ops.gat_layer(x, adj, list(self.out_att), ops.GAT_OUTPUT, len(self.attentions), *drop())
        self.last_seeds = seeds if self.training and self.dropout > 0 else None
        return x


# ------------------------------------------------------------------ Models/BiDAF/wrapper.py:115-151
class GCN(nn.Module):
    """x = relu(linear(A_hat @ x)) per layer, A_hat = D^-1/2 A D^-1/2 with D the row sums of the adjacency values --
    applied as bit rows + per-row scales (ops.GCNAdj), never as a dense matrix."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers=1, dropout=0.5):
        super().__init__()
        _drop_caches_on_load(self)
        self.dropout = dropout
        self.num_layers = num_layers
        self.input_dim = input_dim
        self.output_dim = output_dim
        linears = []
        for num in range(self.num_layers):
            # the reference's quirk, kept: the LAST layer maps to hidden_dim, the others to output_dim
            linears.append(Linear(input_dim, hidden_dim if num == num_layers - 1 else output_dim))
            input_dim = hidden_dim
        self.Linear = nn.ModuleList(linears)
        self.last_seed = None       # input-dropout seed of the last training-mode forward (ops.feat_dropout)

    def forward(self, x, adj):
        """x (B,L,input_dim); adj dense (B,L,L) (weighted: its values are normalised) or PackedAdj."""
        adj = ops.as_packed(adj)
        p, seed = _encoder_drop(self.training, self.dropout)
        self.last_seed = seed if p > 0 else None
        x = ops.feat_dropout(x, p, seed)
        a_hat = ops.GCNAdj(adj)
        for linear in self.Linear:
            x = ops.relu(linear(a_hat.apply(x)))
        return x


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:112-148
class ConcatNotEqualSelfAtt(nn.Module):
    def __init__(self, inp_dim: int, out_dim: int, num_heads: int = 1):
        super().__init__()
        self.inp_dim, self.out_dim, self.num_heads = inp_dim, out_dim, num_heads
        _drop_caches_on_load(self)
        self.linear1 = nn.Linear(inp_dim, out_dim, bias=False)
        self.linear2 = nn.Linear(out_dim, num_heads, bias=False)

    def forward(self, left: torch.Tensor, right: torch.Tensor, mask: torch.Tensor, plan=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """plan (ops.RaggedPlan): `right` / `mask` are node-compact (m_real, D) / (m_real,), weights come back compact."""
        if plan is None:
            assert left.size(0) == right.size(0), "Must same dimensions"
            assert len(left.size()) == 2 and len(right.size()) == 3
        assert self.inp_dim == (left.size(-1) + right.size(-1))
        return ops.concat_att(left, right, mask, self.linear1.weight, self.linear2.weight, plan)


class ConcatSelfAtt(ConcatNotEqualSelfAtt):
    """two_branches_attention.py:73-109 -- identical arithmetic to ConcatNotEqualSelfAtt."""


# ------------------------------------------------------------------ thirdparty/self_attention.py:51-100
class MultiHeadSelfAttentionICLR2017Extend(nn.Module):
    def __init__(self, inp_dim: int, out_dim: int, num_heads: int):
        super().__init__()
        self.inp_dim, self.out_dim, self.num_heads = inp_dim, out_dim, num_heads
        _drop_caches_on_load(self)
        self.linear1 = nn.Linear(inp_dim, out_dim, bias=False)
        self.linear2 = nn.Linear(out_dim, num_heads, bias=False)

    def forward(self, tsr: torch.Tensor, mask: torch.Tensor, return_att_weights=False):
        assert len(tsr.size()) == 3
        assert tsr.size(-1) == self.inp_dim
        attended, weights = ops.concat_att(None, tsr, mask, self.linear1.weight, self.linear2.weight)
        attended = attended.permute(0, 2, 1)       # (B, C, D)
        if return_att_weights:
            return attended, weights
        return attended


# ------------------------------------------------------------------ thirdparty/self_attention.py:8-10
class SelfAttentionType(IntEnum):
    MultiHeadAttentionTanh = 1
    MultiHeadAttentionTransformer = 2


def _query_att_checks(left: torch.Tensor, right: torch.Tensor):
    assert left.size(0) == right.size(0) and left.size(-1) == right.size(-1), "Must same dimensions"
    assert len(left.size()) == 2 and len(right.size()) == 3


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:9-38
class Dot(nn.Module):
    """Attention of `left` (B,D) over `right` (B,L,D) by dot product; returns (avg (B,D), weights (B,L))."""

    def forward(self, left: torch.Tensor, right: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        _query_att_checks(left, right)
        _lib.require_cuda(left, right, mask)
        return ops.query_att(left, right, mask)


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:41-70
class BiLinear(nn.Module):
    """Dot attention with the query W(left)."""

    def __init__(self, dim: int):
        super().__init__()
        _drop_caches_on_load(self)
        self.W = nn.Linear(dim, dim)

    def forward(self, left: torch.Tensor, right: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        _query_att_checks(left, right)
        _lib.require_cuda(left, right, mask)
        return ops.query_att(ops.linear(left, self.W.weight, self.W.bias), right, mask)


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:151-191
class BiLinearTanh(nn.Module):
    """combine(tanh(left_linear(left_tsr) + right_linear(right_tsr))) scores the SEQUENCE `left_tsr` (B,L,H), the first
    argument, against the query `right_tsr` (B,D); returns (attended (B,H), weights (B,L))."""

    def __init__(self, left_dim: int, right_dim: int, out_dim: int):
        super().__init__()
        _drop_caches_on_load(self)
        self.left_linear = nn.Linear(left_dim, out_dim, bias=True)
        self.right_linear = nn.Linear(right_dim, out_dim, bias=False)
        self.combine = nn.Linear(out_dim, 1, bias=False)

    def forward(self, left_tsr: torch.Tensor, right_tsr: torch.Tensor, mask: torch.Tensor):
        assert len(left_tsr.size()) == 3 and len(mask.size()) == 2
        _lib.require_cuda(left_tsr, right_tsr, mask)
        pre = ops.linear(left_tsr, self.left_linear.weight, self.left_linear.bias)
        u = ops.linear(right_tsr, self.right_linear.weight)
        attended, weights = ops.tanh_att(pre, u, self.combine.weight, mask, left_tsr)
        return attended.squeeze(1), weights.squeeze(-1)


# ------------------------------------------------------------------ thirdparty/self_attention.py:13-48
class SelfAttentionICLR2017(nn.Module):
    """Single-head structured self-attention; returns avg (B,D) only.  `num_heads` sizes linear2 as in the reference,
    whose forward works for num_heads == 1 alone (its mask no longer broadcasts otherwise): other values raise here."""

    def __init__(self, inp_dim: int, out_dim: int, num_heads: int = 1):
        super().__init__()
        self.inp_dim, self.out_dim = inp_dim, out_dim
        _drop_caches_on_load(self)
        self.linear1 = nn.Linear(inp_dim, out_dim, bias=False)
        self.linear2 = nn.Linear(out_dim, num_heads, bias=False)

    def forward(self, tsr: torch.Tensor, mask: torch.Tensor):
        assert len(tsr.size()) == 3
        assert tsr.size(-1) == self.inp_dim
        num_heads = self.linear2.weight.shape[0]
        if num_heads != 1:
            raise RuntimeError(f"SelfAttentionICLR2017: num_heads={num_heads}, but the forward is defined for num_heads == 1 only "
                               "(the reference's mask does not broadcast over several heads)")
        _lib.require_cuda(tsr, mask)
        pre = ops.linear(tsr, self.linear1.weight)
        attended, _ = ops.tanh_att(pre, None, self.linear2.weight, mask, tsr)
        return attended.squeeze(1)


# ------------------------------------------------------------------ thirdparty/self_attention.py:103-153
class MultiHeadSelfAttentionICLR17OnWord(nn.Module):
    """Multi-head structured self-attention scored on `tsr` (B,L,D), averaging `original` (B,L,X); returns (B,C,X)."""

    def __init__(self, inp_dim: int, out_dim: int, num_heads: int):
        super().__init__()
        self.inp_dim, self.out_dim, self.num_heads = inp_dim, out_dim, num_heads
        _drop_caches_on_load(self)
        self.linear1 = nn.Linear(inp_dim, out_dim, bias=False)
        self.linear2 = nn.Linear(out_dim, num_heads, bias=False)

    def forward(self, original: torch.Tensor, tsr: torch.Tensor, mask: torch.Tensor, return_att_weights=False):
        assert len(tsr.size()) == 3
        assert tsr.size(-1) == self.inp_dim
        _lib.require_cuda(original, tsr, mask)
        pre = ops.linear(tsr, self.linear1.weight)
        attended, weights = ops.tanh_att(pre, None, self.linear2.weight, mask, original)
        if return_att_weights:
            return attended, weights
        return attended


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:391-422
class ScaledDotProductAttention(nn.Module):
    """softmax(query key^T) value with a bool mask (True = masked); the reference divides by no temperature (:415 is commented
    out) and has no dropout, the two arguments are kept for the signature.  Returns (output (N,Lq,dv), attn (N,Lq,Lk)); masked
    entries of attn are exactly 0 and a fully masked row is all zero."""

    def __init__(self, temperature, attn_dropout=0.1):
        super().__init__()
        self.temperature = temperature

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask=None):
        if mask is None:
            raise TypeError("ScaledDotProductAttention: mask is None, but the forward fills by it (two_branches_attention.py:419)")
        _lib.require_cuda(query, key, value, mask)
        return ops.mha_sdpa(query, key, value, mask, 1)


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:271-347
class MultiHeadAttentionOriginal(nn.Module):
    """Transformer-style multi-head attention with a residual LayerNorm: q (B,Lq,D), k = v (B,Lk,D), mask (B,Lq,Lk) bool with
    True = masked; returns (output (B,Lq,D), None).  The heads stay column slices of the three projections' outputs."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.1):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        _drop_caches_on_load(self)
        self.w_qs = nn.Linear(d_model, n_head * d_k)
        self.w_ks = nn.Linear(d_model, n_head * d_k)
        self.w_vs = nn.Linear(d_model, n_head * d_v)
        self.attention = ScaledDotProductAttention(temperature=np.power(1, 1))
        self.layer_norm = nn.LayerNorm(d_model)
        self.fc = nn.Linear(n_head * d_v, d_model)

    def forward(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: torch.Tensor = None):
        if mask is None:
            raise TypeError("MultiHeadAttentionOriginal: mask is None, but the forward repeats it per head (two_branches_attention.py:337)")
        _lib.require_cuda(q, k, v, mask)
        residual = q
        qp = ops.linear(q, self.w_qs.weight, self.w_qs.bias)
        kp = ops.linear(k, self.w_ks.weight, self.w_ks.bias)
        vp = ops.linear(v, self.w_vs.weight, self.w_vs.bias)
        output, _ = ops.mha_sdpa(qp, kp, vp, mask, self.n_head)
        output = ops.linear(output, self.fc.weight, self.fc.bias)
        output = ops.add_layernorm(output, residual, self.layer_norm.weight, self.layer_norm.bias, self.layer_norm.eps)
        return output, None


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:350-388
class ConcatNotEqualSelfAttTransFormer(nn.Module):
    """Additive attention of one query row over `key`, averaging the separate `value`: query (B,1,X), key (B,L,D), value
    (B,L,Dv), mask (B,1,L) bool with True = PAD (inverted relative to the other attention modules); returns
    (attended (B,Dv,1), weights (B,L,1)).  linear1 over cat([query, key]) splits into the hoisted query branch and the key
    branch of ops.tanh_att.  The reference's expand() admits more query rows only where they equal L and then scores row l
    against key l; that use is not supported: a query with more than one row raises."""

    def __init__(self, inp_dim: int, out_dim: int):
        super().__init__()
        self.inp_dim, self.out_dim = inp_dim, out_dim
        _drop_caches_on_load(self)
        self.linear1 = nn.Linear(inp_dim, out_dim, bias=False)
        self.linear2 = nn.Linear(out_dim, 1, bias=False)

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask: torch.Tensor) \
            -> Tuple[torch.Tensor, torch.Tensor]:
        assert query.size(0) == key.size(0), "Must same dimensions"
        assert self.inp_dim == (query.size(-1) + key.size(-1))
        if query.dim() != 3 or query.size(1) != 1:
            raise RuntimeError(f"ConcatNotEqualSelfAttTransFormer: only a single query row (B,1,X) is supported, got {tuple(query.shape)}")
        _lib.require_cuda(query, key, value, mask)
        x = query.size(-1)
        w1 = self.linear1.weight
        pre = ops.linear(key, w1[:, x:])
        u = ops.linear(query[:, 0], w1[:, :x])
        real = mask.reshape(key.size(0), key.size(1)) == 0
        attended, weights = ops.tanh_att(pre, u, self.linear2.weight, real, value)
        return attended.transpose(1, 2), weights


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:194-268
class MultiHeadAttentionSimple(nn.Module):
    """Multi-head additive attention of `left` (B,X) over `right` (B,L,D), mask (B,L) with 0 = pad; returns
    (tmp (B,1,d_model), weights (num_heads*B, L, 1)), head-major.  An all-padding sequence gives NaN for that sequence."""

    def __init__(self, num_heads: int, d_model: int, d_key: int, d_value: int, init_weights: bool = False,
                 use_layer_norm: bool = False):
        super().__init__()
        self.num_heads = num_heads
        self.d_model, self.d_key, self.d_value = d_model, d_key, d_value
        assert d_model == d_key == d_value
        self.use_layer_norm = use_layer_norm
        _drop_caches_on_load(self)
        self.w_qs = nn.Linear(d_model, num_heads * d_key)
        self.w_ks = nn.Linear(d_model, num_heads * d_key)
        self.w_vs = nn.Linear(d_model, num_heads * d_value)
        if init_weights:
            nn.init.normal_(self.w_qs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_key)))
            nn.init.normal_(self.w_ks.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_key)))
            nn.init.normal_(self.w_vs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_value)))
        self.attention_func = ConcatNotEqualSelfAttTransFormer(inp_dim=(d_key + d_key), out_dim=d_key)
        self.fc = nn.Linear(num_heads * d_value, d_model)
        if init_weights:
            nn.init.xavier_normal_(self.fc.weight)
        if use_layer_norm:
            self.layer_norm = nn.LayerNorm(d_model)

    def forward(self, left: torch.Tensor, right: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        assert left.size(0) == right.size(0), "Must same dimensions"
        assert len(left.size()) == 2 and len(right.size()) == 3
        B, L, D = right.size()
        assert D == self.d_model == self.d_key, "Must have same shape"
        _lib.require_cuda(left, right, mask)
        H, len_q = self.num_heads, 1
        query = ops.linear(left, self.w_qs.weight, self.w_qs.bias).view(B, len_q, H, self.d_key)
        key = ops.linear(right, self.w_ks.weight, self.w_ks.bias).view(B, L, H, self.d_key)
        value = ops.linear(right, self.w_vs.weight, self.w_vs.bias).view(B, L, H, self.d_value)
        # head-major (num_heads * B) sequences: the [b'][l][h] layout ops.tanh_att reads
        q = query.permute(2, 0, 1, 3).contiguous().view(-1, len_q, self.d_key)
        k = key.permute(2, 0, 1, 3).contiguous().view(-1, L, self.d_key)
        v = value.permute(2, 0, 1, 3).contiguous().view(-1, L, self.d_value)
        pad = (mask == 0).unsqueeze(1).repeat(H, 1, 1)
        attended, attention_weights = self.attention_func(query=q, key=k, value=v, mask=pad)
        output = attended.reshape(H, B, len_q, self.d_value).permute(1, 2, 0, 3).contiguous().view(B, len_q, -1)
        tmp = ops.linear(output, self.fc.weight, self.fc.bias)
        if self.use_layer_norm:
            tmp = ops.add_layernorm(tmp, None, self.layer_norm.weight, self.layer_norm.bias, self.layer_norm.eps)
        return tmp, attention_weights


# ------------------------------------------------------------------ thirdparty/two_branches_attention.py:425-430
class CoDaAttention(nn.Module):
    """The reference's empty stub: no parameters, forward returns None."""

    def __init__(self, dim: int):
        super().__init__()

    def forward(self, *input):
        return None


def init_weights(m):
    """torch_utils.py:379-388 (Linear branch): xavier-uniform weight, zero bias."""
    if type(m) == nn.Linear:
        nn.init.xavier_uniform_(m.weight)
        if hasattr(m.bias, "data"):
            m.bias.data.fill_(0)


class _HeadLinear(nn.Linear):
    """nn.Linear whose forward runs the library GEMM (keeps the reference's `out.0.weight` names)."""

    def forward(self, x):
        return ops.linear(x, self.weight, self.bias)


# ------------------------------------------------------------------ Models/FCWithEvidences/graph_based_semantic_structure.py:15-274
class Graph_basedSemantiStructure(nn.Module):
    """GET: claim GGNN + evidence GGNN with GSL + word- and evidence-level concat attention + head."""

    def __init__(self, params):
        super().__init__()
        _drop_caches_on_load(self)
        self._params = params
        self.embedding = self._make_default_embedding_layer(params)
        self.num_classes = params["num_classes"]
        self.fixed_length_right = params["fixed_length_right"]
        self.fixed_length_left = params["fixed_length_left"]
        self.use_claim_source = params["use_claim_source"]
        self.use_article_source = params["use_article_source"]
        self._use_cuda = params["cuda"]
        self.num_att_heads_for_words = params["num_att_heads_for_words"]
        self.num_att_heads_for_evds = params["num_att_heads_for_evds"]
        self.dropout_gnn = params["dropout_gnn"]
        self.dropout_left = params["dropout_left"]
        self.dropout_right = params["dropout_right"]
        self.hidden_size = params["hidden_size"]
        self.output_size = params["output_size"]
        self.gsl_rate = params["gsl_rate"]
        self.num_heads = 1
        H = self.hidden_size
        if self.use_claim_source:
            self.claim_source_embs = self._make_entity_embedding_layer(params["claim_source_embeddings"], freeze=False)
            self.claim_emb_size = params["claim_source_embeddings"].shape[1]
        if self.use_article_source:
            self.article_source_embs = self._make_entity_embedding_layer(params["article_source_embeddings"], freeze=False)
            self.article_emb_size = params["article_source_embeddings"].shape[1]
        D = params["embedding_output_dim"]
        # the recurrent encoders of BasicFCModel.__init__ (basic_fc_model.py:49-52): GET's forward never runs them; they keep
        # nn.LSTM's own init here so that a seeded construction of the model draws what it always drew
        self.bilstm = LSTM(input_size=D, hidden_size=H, num_layers=1, bidirectional=True, batch_first=True,
                           dropout=self.dropout_left, _reset_params=False)
        self.query_bilstm = LSTM(input_size=D, hidden_size=H, num_layers=1, bidirectional=True, batch_first=True,
                                 dropout=self.dropout_right, _reset_params=False)
        # live graph encoders (:52-55)
        self.ggnn4claim_1 = GGNN(in_features=D, out_features=H)
        self.ggnn_with_gsl = GGNN_with_GSL(input_dim=D, hidden_dim=H, output_dim=H, rate=self.gsl_rate,
                                           dropout=self.dropout_gnn)
        self.trans = Linear(2 * H, H)          # constructed, never used (:55)
        # attention (:223-249)
        self.self_att_word = ConcatNotEqualSelfAtt(inp_dim=2 * H, out_dim=H, num_heads=self.num_att_heads_for_words)
        evd_inp = H + self.num_att_heads_for_words * H
        if self.use_claim_source:
            evd_inp += self.claim_emb_size
        if self.use_article_source:
            evd_inp += self.article_emb_size
        self.self_att_evd = ConcatNotEqualSelfAtt(inp_dim=evd_inp, out_dim=H, num_heads=self.num_att_heads_for_evds)
        # head (:62-74): Linear -> Linear, no activation
        evd_input_size = H
        if self.use_claim_source:
            evd_input_size += self.claim_emb_size
        evd_input_size += H * self.num_att_heads_for_words * self.num_att_heads_for_evds
        if self.use_article_source:
            evd_input_size += self.article_emb_size * self.num_att_heads_for_evds
        self.out = nn.Sequential(_HeadLinear(evd_input_size, H), _HeadLinear(H, self.output_size))
        for m in self.out:
            nn.init.xavier_uniform_(m.weight)
            m.bias.data.fill_(0)

    # -- Models/base_model.py:144-162,184-188
    @staticmethod
    def _make_default_embedding_layer(_params) -> nn.Module:
        if isinstance(_params["embedding"], np.ndarray):
            _params["embedding_input_dim"] = _params["embedding"].shape[0]
            _params["embedding_output_dim"] = _params["embedding"].shape[1]
            return Embedding.from_pretrained(embeddings=torch.Tensor(_params["embedding"]),
                                             freeze=_params["embedding_freeze"])
        return Embedding(num_embeddings=_params["embedding_input_dim"],
                         embedding_dim=_params["embedding_output_dim"])

    @staticmethod
    def _make_entity_embedding_layer(matrix: np.ndarray, freeze: bool) -> nn.Module:
        return Embedding.from_pretrained(embeddings=torch.Tensor(matrix), freeze=freeze)

    # -- forward (:76-125)
    def forward(self, query: torch.Tensor, document: torch.Tensor, verbose=False, **kargs):
        K = KeyWordSettings
        assert K.Query_lens in kargs and K.Doc_lens in kargs
        B, L = query.size()
        assert query.size(0) == document.size(0)
        batch_size, n, R = document.size()
        assert n == 30
        assert K.DocContentNoPaddingEvidence in kargs
        doc = kargs[K.DocContentNoPaddingEvidence]               # (B1, R) de-padded evidence node ids
        if K.DocLensIndices in kargs and kargs[K.DocLensIndices] is not None:
            d_lens = kargs[K.DocLensIndices][2]
            assert d_lens.shape[0] == doc.size(0)
        b1 = doc.size(0)
        n_max = kargs[K.FIXED_NUM_EVIDENCES]
        # The whole forward (and, through autograd, the whole backward) as ONE library call each when the model and
        # the batch qualify (get_amd/fused.py: fp32, frozen word table, float4-shaped widths with d <= h <= 320); the
        # module-by-module path below is the general one.
        from . import fused
        if _lib.gemm_mode() == "fp32x3p":
            ops.fp32x3p_guard(self)
        if fused.eligible(self, query, kargs):
            phi, word_w, evd_att_weight, plan = fused.forward(self, query, document, kargs)
            if kargs.get(K.OutputRankingKey, False):
                hw = self.num_att_heads_for_words
                word_att_weights = plan.to_padded(word_w) if plan is not None else word_w.view(b1, R, hw)
                return phi, (word_att_weights, evd_att_weight)
            return phi
        seg = ops.Segments(kargs[K.EvidenceCountPerQuery], b1, n_max)

        # claim branch (:144-155): GGNN -> masked mean over the unique claim nodes -> one row per pair
        def claim_branch():
            q_hid = self.ggnn4claim_1.forward_ids(kargs[K.Query_Adj], self.embedding, query)
            q = ops.masked_mean(q_hid, query, kargs[K.Query_lens])             # (B, H)
            return q, ops.seg_broadcast(q, seg)                                # (B1, H)

        # The claim branch is a chain of few-row launches (B x L rows) that is independent of the evidence branch until
        # the word attention: on a ROCm device it runs on a side stream underneath the evidence cells' GEMMs.  It is
        # issued AFTER the evidence branch so that autograd (which replays nodes newest-first, each on its forward
        # stream) also starts the claim backward before the evidence cells' backward.
        side = ops.side_stream(query.device) if ops.streams.CLAIM_SIDE_STREAM and query.is_cuda else None
        if side is None:
            q_repr, query_repr = claim_branch()
        else:
            main = torch.cuda.current_stream(query.device)
            inputs_ready = torch.cuda.Event()
            inputs_ready.record(main)

        # evidence branch (:107): GGNN -> scorer + GSL -> GGNN on the refined graph.  A PackedAdj that carries a
        # node-compact plan (NativeBatch) takes the fast path that skips the padding nodes wherever they cannot
        # influence a result (ops.RaggedPlan); anything else runs the reference's padded layout.
        d_adj = kargs[K.Evd_Docs_Adj]
        plan = d_adj.plan if isinstance(d_adj, PackedAdj) else None
        doc_out = self.ggnn_with_gsl.forward_ids(d_adj, self.embedding, doc, plan=plan)

        if side is not None:
            side.wait_event(inputs_ready)
            with torch.cuda.stream(side):
                q_repr, query_repr = claim_branch()
            main.wait_stream(side)
            q_repr.record_stream(main)
            query_repr.record_stream(main)
            if query_repr.requires_grad:
                # the claim branch's backward will run on the side stream: join it at the end of the backward pass
                # whether or not any other side-stream work (ops.streams._side_wgrad) happens in that pass
                dev_ = query.device
                query_repr.register_hook(lambda g, _d=dev_: ops.side_mark_backward(_d))

        # word-level attention (:173-193); the claim vector WITHOUT its source embedding (:110)
        if plan is None:
            att, word_att_weights = self.self_att_word(query_repr, doc_out, doc >= 1)
        else:
            att, word_w = self.self_att_word(query_repr, doc_out, plan.maskf[:plan.m_real], plan=plan)
            word_att_weights = None
        avg = torch.flatten(att, start_dim=1)                                   # (B1, H*hw), head fastest

        # evidence-level attention (:195-221).  Its left input is row 0 of pad_right([claim source | query_repr]), i.e. the
        # claim's own vector (zeros for a claim without evidences) -- taken per claim instead of broadcasting to B1 pairs,
        # padding to (B, n, X) and slicing slot 0
        left_claim = q_repr
        if self.use_claim_source:
            claim_embs = self.claim_source_embs(kargs[K.QuerySources].long()).squeeze(1)
            left_claim = torch.cat([claim_embs, q_repr], dim=-1)                # source first (:116)
        new_left = left_claim * seg.has                                         # (B, X)
        # pad_right(avg) ++ article_source_embs(src with -1 -> 0) and the slot mask, one launch (:157-170, :195-215)
        padded_avg, mask = ops.evd_assemble(avg, self.article_source_embs.weight if self.use_article_source else None, seg,
                                            kargs[K.DocSources] if self.use_article_source else None, document)
        attended_avg, evd_att_weight = self.self_att_evd(new_left.contiguous(), padded_avg, mask)
        output = torch.cat([new_left, torch.flatten(attended_avg, start_dim=1)], dim=-1)   # (:251-267)
        phi = self.out(output)
        if kargs.get(K.OutputRankingKey, False):
            if word_att_weights is None:
                word_att_weights = plan.to_padded(word_w)          # (B1, R, hw), zeros at the padding nodes
            return phi, (word_att_weights, evd_att_weight)
        return phi

    def predict(self, query: torch.Tensor, doc: torch.Tensor, verbose: bool = False, **kargs):
        self.train(False)
        assert query.size(0) == doc.size(0)
        return self(query, doc, **kargs)

    # ragged helpers kept under the reference's names (basic_fc_model.py:80-121)
    def _pad_left_tensor(self, left_tsr: torch.Tensor, **kargs):
        cnt = kargs[KeyWordSettings.EvidenceCountPerQuery]
        b1 = int(cnt.sum().item())
        return ops.seg_broadcast(left_tsr, ops.Segments(cnt, b1, kargs.get(KeyWordSettings.FIXED_NUM_EVIDENCES, 30)))

    @classmethod
    def _pad_right_tensor(cls, tsr: torch.Tensor, **kargs):
        cnt = kargs[KeyWordSettings.EvidenceCountPerQuery]
        return ops.seg_pad(tsr, ops.Segments(cnt, tsr.size(0), kargs[KeyWordSettings.FIXED_NUM_EVIDENCES]))


# ------------------------------------------------------------------ Models/BiDAF/bidaf_model.py:11-172
class BiDAF(nn.Module):
    """The reference's BiDAF sequence-matching baseline on the HIP kernels: the highway gate and the attention-flow layer of
    csrc/bidaf_ops.hip (ops.highway, ops.att_flow), the LSTM drop-in for the two encoders, ops.linear for every projection.

    params keys read (the reference's, no others): ``embedding`` (a numpy matrix) or ``embedding_input_dim`` /
    ``embedding_output_dim``, ``embedding_freeze``, ``word_dim``, ``hidden_size``, ``dropout``; the two dims are written back
    into params when a matrix is given, as BaseModel._make_default_embedding_layer does.  Submodule names, order, shapes and
    inits are the reference's, so state_dict() matches key for key.  The nn.Sequential(Linear, ReLU | Sigmoid) holders of the
    highway layers only keep those keys: the forward calls their Linear and folds the activation into ops.highway.

    forward(query (B,L) ids, document (B,R) ids, query_lens_indices=(new_indices, restoring_indices, lens),
    doc_lens_indices=(...)) -> (B, 1).  Both sides are encoded to max(lens) steps, as pad_packed_sequence leaves them.
    The attention-flow layer has NO mask, as in the reference: the encoder's exact-zero rows at t >= len take part in both
    softmaxes.  Where the reference's .squeeze() calls break it -- B == 1 raises there, a context of length 1 broadcasts to a
    wrong shape -- this class computes the layer's formulas (ops.att_flow); it emulates neither.  The gradients of the three
    attention biases are mathematically zero and arrive as exact zeros.  Limits (ops.att_flow): context and query length <=
    1024, hidden_size <= 1024.
    Training mode: the only dropout sites are the input dropouts of the three LSTM calls; their seeds are kept in
    ``last_seeds`` (context encoder on the document, context encoder on the query, modeling encoder), since the second call
    of ``context_LSTM`` overwrites its ``last_seed``."""

    def __init__(self, params):
        super().__init__()
        _drop_caches_on_load(self)
        self._params = params
        self.word_emb = Graph_basedSemantiStructure._make_default_embedding_layer(params)
        D, H = params["word_dim"], params["hidden_size"]
        for i in range(2):
            setattr(self, "highway_linear%s" % i, nn.Sequential(Linear(D, D), nn.ReLU()))
            setattr(self, "highway_gate%s" % i, nn.Sequential(Linear(D, D), nn.Sigmoid()))
        self.context_LSTM = LSTM(input_size=D, hidden_size=H, bidirectional=True, batch_first=True, dropout=params["dropout"])
        self.att_weight_c = Linear(H * 2, 1)
        self.att_weight_q = Linear(H * 2, 1)
        self.att_weight_cq = Linear(H * 2, 1)
        self.modeling_LSTM1 = LSTM(input_size=H * 8, hidden_size=H, bidirectional=True, batch_first=True, dropout=params["dropout"])
        self.dropout = nn.Dropout(p=params["dropout"])      # constructed, never applied (:45)
        self.last_linear = _HeadLinear(2 * H, 1)
        self.last_seeds = [None, None, None]

    def _highway(self, x):
        for i in range(2):
            h_pre = getattr(self, "highway_linear%s" % i)[0](x)
            g_pre = getattr(self, "highway_gate%s" % i)[0](x)
            x = ops.highway(x, h_pre, g_pre)
        return x

    def forward(self, query: torch.Tensor, document: torch.Tensor, verbose=False, **kargs):
        q_new, q_restoring, q_lens = kargs["query_lens_indices"]
        d_new, d_restoring, c_lens = kargs["doc_lens_indices"]
        q_word = self.word_emb(query.long())
        c_word = self.word_emb(document.long())
        _lib.require_cuda(q_word, c_word)
        c = self._highway(c_word)
        q = self._highway(q_word)
        c = self.context_LSTM((c, c_lens, d_new, d_restoring))[0]
        seed_c = self.context_LSTM.last_seed
        q = self.context_LSTM((q, q_lens, q_new, q_restoring))[0]
        seed_q = self.context_LSTM.last_seed
        att = self.att_weight_c.linear, self.att_weight_q.linear, self.att_weight_cq.linear
        g = ops.att_flow(c, q, att[0].weight, att[1].weight, att[2].weight, att[0].bias, att[1].bias, att[2].bias)
        m = self.modeling_LSTM1((g, c_lens, d_new, d_restoring))[1]
        self.last_seeds = [seed_c, seed_q, self.modeling_LSTM1.last_seed]
        return self.last_linear(m)

    def predict(self, query, doc, verbose: bool = False, **kargs):
        assert KeyWordSettings.Query_lens in kargs and KeyWordSettings.Doc_lens in kargs
        self.train(False)
        dev = self.word_emb.weight.device

        def lens_indices(lens):
            lens = lens.detach().cpu().numpy() if torch.is_tensor(lens) else np.array(lens)
            new = np.argsort(-lens)             # torch_utils.get_sorted_index_and_reverse_index: descending lengths and
            return new, np.argsort(new), lens   # the permutation that restores the original order
        out = self(torch.as_tensor(query).to(dev), torch.as_tensor(doc).to(dev), verbose=False,
                   query_lens_indices=lens_indices(kargs[KeyWordSettings.Query_lens]),
                   doc_lens_indices=lens_indices(kargs[KeyWordSettings.Doc_lens]))
        return out.detach().cpu().numpy().flatten()


# ------------------------------------------------------------------ matchzoo/modules/attention.py:9-38
class Attention(nn.Module):
    """softmax(linear(x)) over the kept positions (ops.lin_att): x (B,L,input_size) -> (B,L).  ``mask`` is the reference's
    integer, read as its two comparisons read it -- ``mask = (s != m)`` and ``masked_fill(mask == m, -inf)`` on the scores s:
    m == 0 (the default) excludes the positions that score exactly 0 (all-zero rows of x), m == 1 excludes every position that
    does not score exactly 1, and any other m excludes nothing.  A sequence without a kept position is NaN in its own row."""

    def __init__(self, input_size: int = 100, mask: int = 0):
        super().__init__()
        self.linear = nn.Linear(input_size, 1, bias=False)
        self.mask = mask

    def forward(self, x):
        mode = 0 if self.mask == 0 else (1 if self.mask == 1 else 2)
        return ops.lin_att(x, self.linear.weight, mode)


# ------------------------------------------------------------------ matchzoo/modules/attention.py:41-65
class BidirectionalAttention(nn.Module):
    """Soft attention between two sequences, both ways (ops.soft_align twice): forward(v1 (B,L1,D), v1_mask (B,L1), v2
    (B,L2,D), v2_mask (B,L2)) -> attended_v1 (B,L1,D), attended_v2 (B,L2,D).  The masks are bool, True = padding (any other
    dtype raises RuntimeError, as torch's masked_fill does).  As in the reference a padded key is NOT excluded: its score is
    replaced by -1e-7 and it keeps a weight; only the padded ROWS of the two results are zeroed."""

    def __init__(self):
        super().__init__()

    def forward(self, v1, v1_mask, v2, v2_mask):
        for m in (v1_mask, v2_mask):
            if m.dtype != torch.bool:
                raise RuntimeError(f"BidirectionalAttention: masked_fill only supports boolean masks, but got mask with dtype {m.dtype}")
        attended_v1 = ops.soft_align(v1, v2, v2, v2_mask, row_zero=v1_mask)[0]
        # the reference's softmax(dim=1) branch, transposed
        attended_v2 = ops.soft_align(v2, v1, v1, v1_mask, row_zero=v2_mask)[0]
        return attended_v1, attended_v2


# ------------------------------------------------------------------ matchzoo/modules/attention.py:68-107
class MatchModule(nn.Module):
    """The match representation of Match-LSTM: forward(v1 (B,L1,H), v2 (B,L2,H), v2_mask (B,L2), any dtype, nonzero =
    padding) -> (B,L1,2H) = dropout(relu(proj([v1, o, v1 - o, v1 * o]))), o = softmax(fill(v1 v2_proj(v2)^T)) v2.  The
    alignment and the four-way cat are one kernel (ops.soft_align with fuse); padded keys keep a weight (score -1e-7), as in
    the reference.  Training mode with dropout_rate > 0: the stateless mask of ops.feat_dropout, seed kept in ``last_seed``."""

    def __init__(self, hidden_size, dropout_rate=0):
        super().__init__()
        _drop_caches_on_load(self)
        self.v2_proj = nn.Linear(hidden_size, hidden_size)
        self.proj = nn.Linear(hidden_size * 4, hidden_size * 2)
        self.dropout = nn.Dropout(p=dropout_rate)
        self.last_seed = None

    def forward(self, v1, v2, v2_mask):
        _lib.require_cuda(v1, v2, v2_mask)
        proj_v2 = ops.linear(v2, self.v2_proj.weight, self.v2_proj.bias)
        fusion = ops.soft_align(v1, proj_v2, v2, v2_mask != 0, fuse=True)[0]
        match = ops.relu(ops.linear(fusion, self.proj.weight, self.proj.bias))
        p, seed = _encoder_drop(self.training, self.dropout.p)
        self.last_seed = seed if p > 0 else None
        return ops.feat_dropout(match, p, seed)


# ------------------------------------------------------------------ matchzoo/modules/matching.py:9-61
class Matching(nn.Module):
    """The matching matrix between two sequences: forward(x (B,L,D), y (B,R,D)) -> (B,L,R) for 'dot' (ops.match_dot; the
    cosine with normalize, where a row with a norm <= 1e-12 gets gradients of the order 1e12, as F.normalize gives), and
    (B,L,R,D) for 'mul', 'plus', 'minus', (B,L,R,2D) for 'concat' (ops.match_bcast)."""

    def __init__(self, normalize: bool = False, matching_type: str = 'dot'):
        super().__init__()
        self._normalize = normalize
        self._validate_matching_type(matching_type)
        self._matching_type = matching_type

    @classmethod
    def _validate_matching_type(cls, matching_type: str = 'dot'):
        valid_matching_type = ['dot', 'mul', 'plus', 'minus', 'concat']
        if matching_type not in valid_matching_type:
            raise ValueError("%s is not a valid matching type, %s expected." % (matching_type, valid_matching_type))

    def forward(self, x, y):
        if self._matching_type == 'dot':
            return ops.match_dot(x, y, self._normalize)
        return ops.match_bcast(x, y, self._matching_type)


# ------------------------------------------------------------------ matchzoo/modules/gaussian_kernel.py:8-36
class GaussianKernel(nn.Module):
    """exp(-0.5 (x - mu)^2 / sigma^2), elementwise (ops.gauss_kernel); sigma == 0 raises at the first forward."""

    def __init__(self, mu: float = 1., sigma: float = 1.):
        super().__init__()
        self.mu = mu
        self.sigma = sigma

    def forward(self, x):
        return ops.gauss_kernel(x, self.mu, self.sigma)


# ------------------------------------------------------------------ matchzoo/modules/dropout.py:4-18
class RNNDropout(nn.Dropout):
    """Dropout of whole feature columns of a sequence batch: forward(x (B,L,D)).  Eval mode returns the input.  Training mode
    draws ONE (B,D) mask, shared by all L positions and scaled by 1 / (1 - p), with the stateless hash of ops.feat_dropout on
    a tensor of ones; its seed is kept in ``last_seed``, so ops.dropout_mask_reference(seed, B, D, p) replays it."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.last_seed = None

    def forward(self, sequences_batch):
        p, seed = _encoder_drop(self.training, self.p)
        self.last_seed = seed if p > 0 else None
        if p <= 0:
            return sequences_batch
        _lib.require_cuda(sequences_batch)
        ones = sequences_batch.new_ones((sequences_batch.shape[0], sequences_batch.shape[-1]), dtype=torch.float32)
        return ops.feat_dropout(ones, p, seed).unsqueeze(1) * sequences_batch


# ------------------------------------------------------------------ matchzoo/modules/stacked_brnn.py:6-91
class StackedBRNN(nn.Module):
    """Stacked bidirectional LSTM / GRU layers with the option to concatenate the layers' outputs, on the HIP recurrence
    kernels.  ``self.rnns`` holds one ``rnn_type(in, hidden, num_layers=1, bidirectional=True)`` per layer as a holder of
    parameters (state_dict keys ``rnns.{i}.weight_ih_l0`` ..., drawn as the reference draws them); the holders are never
    called.  rnn_type is nn.LSTM or nn.GRU, anything else raises TypeError.

    forward(x (B,L,D), x_mask) -> (B,L,2H), or (B,L,layers*2H) with concat_layers.  Every sequence runs over its full length
    L: the reference's _forward_unpadded ignores the padding, and so does this; x_mask is accepted and NOT read (the
    reference's ``x_mask.data.sum() == 0`` is a host synchronisation whose result it discards).  Each layer is the input
    projection (ops.linear) and the recurrence (ops.lstm_seq / ops.gru_seq) of modules.LSTM / modules.GRU, whose limits apply.
    Training mode with dropout_rate > 0: ops.feat_dropout on every layer's input, seeds kept in ``last_seeds`` (one per
    layer), and with dropout_output on the result, seed kept in ``last_output_seed``."""

    def __init__(self, input_size, hidden_size, num_layers, dropout_rate=0, dropout_output=False, rnn_type=nn.LSTM,
                 concat_layers=False):
        super().__init__()
        if rnn_type not in (nn.LSTM, nn.GRU):
            raise TypeError("StackedBRNN: rnn_type must be nn.LSTM or nn.GRU, got %r" % (rnn_type,))
        _drop_caches_on_load(self)
        self.dropout_output = dropout_output
        self.dropout_rate = dropout_rate
        self.num_layers = num_layers
        self.concat_layers = concat_layers
        self.rnns = nn.ModuleList()
        for i in range(num_layers):
            input_size = input_size if i == 0 else 2 * hidden_size
            self.rnns.append(rnn_type(input_size, hidden_size, num_layers=1, bidirectional=True))
        self._layer_fn = _lstm_layer if rnn_type is nn.LSTM else _gru_layer
        self.last_seeds = [None] * num_layers
        self.last_output_seed = None

    def forward(self, x, x_mask=None):
        _lib.require_cuda(x)
        assert x.dim() == 3, "StackedBRNN: x is (B, L, D)"
        B, L = x.shape[0], x.shape[1]
        lens = torch.full((B,), L, device=x.device, dtype=torch.int32)
        outputs, inp = [], x
        for i, rnn in enumerate(self.rnns):
            p, seed = _encoder_drop(self.training, self.dropout_rate)
            self.last_seeds[i] = seed if p > 0 else None
            inp = ops.feat_dropout(inp, p, seed)
            inp = self._layer_fn(lambda kind, sfx: getattr(rnn, "%s_l0%s" % (kind, sfx)), ("", "_reverse"), inp, lens, None, L)[0]
            outputs.append(inp)
        output = torch.cat(outputs, 2) if self.concat_layers else outputs[-1]
        p, seed = _encoder_drop(self.training and self.dropout_output, self.dropout_rate)
        self.last_output_seed = seed if p > 0 else None
        return ops.feat_dropout(output, p, seed).contiguous()


# ------------------------------------------------------------------ matchzoo/losses/rank_hinge_loss.py:7-86
class RankHingeLoss(nn.Module):
    """forward(y_pred (B (num_neg + 1), c), y_true) -> the hinge loss max(0, margin - (pos - mean of the negatives)) of every
    instance (its positive row and the num_neg rows behind it; ops.rank_hinge), reduced by 'none' (B, c), 'mean' or 'sum'.
    y_true is not read, as in the reference, and may be None."""

    __constants__ = ['num_neg', 'margin', 'reduction']

    def __init__(self, num_neg: int = 1, margin: float = 1., reduction: str = 'mean'):
        super().__init__()
        self.num_neg = num_neg
        self.margin = margin
        self.reduction = reduction

    def forward(self, y_pred, y_true=None):
        return ops.rank_hinge(y_pred, self.num_neg, self.margin, self.reduction)

    @property
    def num_neg(self):
        return self._num_neg

    @num_neg.setter
    def num_neg(self, value):
        self._num_neg = value

    @property
    def margin(self):
        return self._margin

    @margin.setter
    def margin(self, value):
        self._margin = value


# ------------------------------------------------------------------ matchzoo/losses/rank_cross_entropy_loss.py:7-48
class RankCrossEntropyLoss(nn.Module):
    """forward(y_pred, y_true (B (num_neg + 1), c)) -> -mean over the instances of sum(labels * log_softmax(logits)), logits and
    labels being the instance's num_neg + 1 rows side by side (ops.rank_cross_entropy).

    One deviation: the reference takes log(softmax(x)), which is -inf for a logit some 104 below its row maximum and NaN under
    a zero label (logits [0, -200] with labels [1, 0] give nan); the stable log-softmax here returns the finite value."""

    __constants__ = ['num_neg']

    def __init__(self, num_neg: int = 1):
        super().__init__()
        self.num_neg = num_neg

    def forward(self, y_pred, y_true):
        return ops.rank_cross_entropy(y_pred, y_true, self.num_neg)

    @property
    def num_neg(self):
        return self._num_neg

    @num_neg.setter
    def num_neg(self, value):
        self._num_neg = value


# ------------------------------------------------------------------ matchzoo/modules/bert_module.py:9-30 (get_amd/bert.py)
from .bert import BertConfig, BertModel, BertModule  # noqa: E402,F401
from .bert import (BertForMaskedLM, BertForMultipleChoice, BertForNextSentencePrediction, BertForPreTraining,  # noqa: E402,F401
                   BertForQuestionAnswering, BertForSequenceClassification, BertForTokenClassification, BertLMPredictionHead,
                   BertOnlyMLMHead, BertOnlyNSPHead, BertPredictionHeadTransform, BertPreTrainingHeads)
