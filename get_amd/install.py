"""``sys.modules`` shims: the reference's module paths -> get_amd's drop-in classes."""
import sys
import types


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__get_amd_shim__ = True
    sys.modules[name] = m
    return m


def install(bert: bool = False):
    """bert: also serve ``matchzoo.modules.BertModule`` (get_amd/bert.py).  Off by default: a plain install() keeps serving
    exactly what it served before, where ``from matchzoo.modules import BertModule`` raises ImportError and callers that probe
    for it fall back; the vendored pytorch_transformers is never shimmed."""
    import numpy as np
    import torch
    import torch.nn as nn

    from . import modules as M
    from .keywords import KeyWordSettings

    # Models.BiDAF.wrapper  (master_get -> graph_based_semantic_structure.py:8)
    _module("Models.BiDAF.wrapper", GGNN=M.GGNN, GGNN_with_GSL=M.GGNN_with_GSL, GSL=M.GSL, Linear=M.Linear,
            LSTM=M.LSTM, GRU=M.GRU, GraphAttentionLayer=M.GraphAttentionLayer, GAT=M.GAT, GCN=M.GCN, torch=torch, nn=nn)
    # thirdparty.two_branches_attention is star-imported by the model module (:9), which is also
    # where that module gets `nn` and `np` from
    _module("thirdparty.two_branches_attention", ConcatNotEqualSelfAtt=M.ConcatNotEqualSelfAtt,
            ConcatSelfAtt=M.ConcatSelfAtt, Dot=M.Dot, BiLinear=M.BiLinear, BiLinearTanh=M.BiLinearTanh,
            ScaledDotProductAttention=M.ScaledDotProductAttention, MultiHeadAttentionOriginal=M.MultiHeadAttentionOriginal,
            ConcatNotEqualSelfAttTransFormer=M.ConcatNotEqualSelfAttTransFormer,
            MultiHeadAttentionSimple=M.MultiHeadAttentionSimple, CoDaAttention=M.CoDaAttention,
            torch=torch, nn=nn, np=np)
    _module("thirdparty.self_attention", MultiHeadSelfAttentionICLR2017Extend=M.MultiHeadSelfAttentionICLR2017Extend,
            SelfAttentionICLR2017=M.SelfAttentionICLR2017,
            MultiHeadSelfAttentionICLR17OnWord=M.MultiHeadSelfAttentionICLR17OnWord, SelfAttentionType=M.SelfAttentionType)
    # the model itself (master_get.py:5,145)
    _module("Models.FCWithEvidences.graph_based_semantic_structure",
            Graph_basedSemantiStructure=M.Graph_basedSemantiStructure, KeyWordSettings=KeyWordSettings)
    # the sequence-matching baseline built from wrapper.LSTM / wrapper.Linear
    _module("Models.BiDAF.bidaf_model", BiDAF=M.BiDAF, LSTM=M.LSTM, Linear=M.Linear, KeyWordSettings=KeyWordSettings,
            torch=torch, nn=nn, np=np)
    # the parts sequence-matching baselines are assembled from (basic_fc_model.py:6 imports GaussianKernel from here).
    # BertModule (a local directory or a BertConfig, get_amd/bert.py) only on request: install(bert=True)
    _module("matchzoo.modules", Attention=M.Attention, BidirectionalAttention=M.BidirectionalAttention,
            MatchModule=M.MatchModule, RNNDropout=M.RNNDropout, StackedBRNN=M.StackedBRNN, GaussianKernel=M.GaussianKernel,
            Matching=M.Matching, torch=torch, nn=nn, **({"BertModule": M.BertModule} if bert else {}))
    # what those baselines train against and are scored with.  The base fitter imports the metric SUBMODULES
    # (Fitting/densebaseline_fit.py:19-20), so every file of matchzoo/metrics and matchzoo/losses is served under its own name
    from . import ranking as R
    by_file = {"precision": R.Precision, "average_precision": R.AveragePrecision,
               "mean_average_precision": R.MeanAveragePrecision, "mean_reciprocal_rank": R.MeanReciprocalRank,
               "discounted_cumulative_gain": R.DiscountedCumulativeGain,
               "normalized_discounted_cumulative_gain": R.NormalizedDiscountedCumulativeGain}
    subs = {name: _module("matchzoo.metrics." + name, BaseMetric=R.BaseMetric, np=np, **{cls.__name__: cls})
            for name, cls in by_file.items()}
    _module("matchzoo.metrics", **subs, **{cls.__name__: cls for cls in by_file.values()})
    losses = {"rank_hinge_loss": M.RankHingeLoss, "rank_cross_entropy_loss": M.RankCrossEntropyLoss}
    subs = {name: _module("matchzoo.losses." + name, torch=torch, nn=nn, **{cls.__name__: cls}) for name, cls in losses.items()}
    _module("matchzoo.losses", **subs, **{cls.__name__: cls for cls in losses.values()})
    return M
