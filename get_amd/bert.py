"""The BERT encoder as a drop-in: ``BertConfig``, ``BertModel`` (pytorch_transformers/modeling_bert.py:142-375, 532-631) and
``BertModule`` (matchzoo/modules/bert_module.py:9-30), backed by csrc/bert_ops.hip and the project's linear, LayerNorm,
embedding and dropout kernels.

``BertModel`` has the reference's module tree, so a reference checkpoint loads unchanged: 5 + 16 * layers + 2 state_dict
keys under ``embeddings.*``, ``encoder.layer.N.*`` and ``pooler.dense.*``.  The attention probabilities are never materialised
(ops.bert_attention), which is why ``output_attentions`` and ``head_mask`` are refused.  Nothing is ever downloaded: a
pretrained model is a local directory holding ``config.json`` and ``pytorch_model.bin``.
"""
from __future__ import annotations

import copy
import json
import math
import os
import warnings

import torch
import torch.nn as nn

from . import _lib, ops

CONFIG_NAME = "config.json"
WEIGHTS_NAME = "pytorch_model.bin"
_ACTS = ("gelu", "relu")


# (field, default) of a configuration, under the reference's field names (configuration_bert.py, configuration_utils.py): the one
# table the constructor, the json reader and to_dict walk
_FIELDS = (
    ("vocab_size", 30522), ("hidden_size", 768), ("num_hidden_layers", 12), ("num_attention_heads", 12), ("intermediate_size", 3072),
    ("hidden_act", "gelu"), ("hidden_dropout_prob", 0.1), ("attention_probs_dropout_prob", 0.1), ("max_position_embeddings", 512),
    ("type_vocab_size", 2), ("initializer_range", 0.02), ("layer_norm_eps", 1e-12),
    ("output_hidden_states", False), ("output_attentions", False), ("num_labels", 2), ("finetuning_task", None),
    ("torchscript", False), ("pruned_heads", {}),
)
_FIELD_NAMES = tuple(name for name, _ in _FIELDS)


class BertConfig:
    """The configuration of a BertModel under the reference's field names (_FIELDS).  `source` is a vocabulary size, the path
    of a config.json, a dict of fields, or None; keyword arguments set single fields on top of it.  Keys of a file or dict
    that are no field are kept as attributes, so a config.json written elsewhere round-trips; an unknown keyword is an error."""

    def __init__(self, source=None, **fields):
        unknown = sorted(set(fields) - set(_FIELD_NAMES))
        if unknown:
            raise TypeError(f"BertConfig: unknown arguments {unknown} (the fields are {list(_FIELD_NAMES)})")
        if isinstance(source, (str, os.PathLike)):
            with open(source, encoding="utf-8") as fh:
                values = json.load(fh)
        elif isinstance(source, dict):
            values = dict(source)
        elif isinstance(source, int) and not isinstance(source, bool):
            values = {"vocab_size": source}
        elif source is None:
            values = {}
        else:
            raise ValueError(f"BertConfig: the first argument is a vocabulary size, a dict of fields or the path of a {CONFIG_NAME}, "
                             f"got {type(source).__name__}")
        values.update(fields)
        for name, default in _FIELDS:
            setattr(self, name, values.pop(name, copy.deepcopy(default)))
        for name, value in values.items():      # what a foreign file holds beyond the fields
            setattr(self, name, value)

    @classmethod
    def from_dict(cls, fields):
        return cls(dict(fields))

    @classmethod
    def from_json_file(cls, path):
        return cls(path)

    def to_dict(self):
        return copy.deepcopy(vars(self))

    def to_json_string(self):
        return json.dumps(self.to_dict(), indent=1, sort_keys=True) + "\n"

    def save_pretrained(self, directory):
        """Writes <directory>/config.json."""
        if not os.path.isdir(directory):
            raise ValueError(f"BertConfig.save_pretrained: {directory!r} is not an existing directory")
        with open(os.path.join(directory, CONFIG_NAME), "w", encoding="utf-8") as fh:
            fh.write(self.to_json_string())

    def __eq__(self, other):
        return isinstance(other, BertConfig) and vars(self) == vars(other)

    def __repr__(self):
        return f"BertConfig({self.to_dict()})"


def _check_config(config: BertConfig):
    """What the kernels cannot serve is refused where the model is built (and again in forward, for a config edited later)."""
    if config.hidden_size % config.num_attention_heads != 0:
        raise ValueError(f"BertModel: hidden_size {config.hidden_size} is not divisible by num_attention_heads "
                         f"{config.num_attention_heads}")
    if config.output_attentions:
        raise ValueError("BertModel: output_attentions is not supported: the attention probabilities are never materialised "
                         "(ops.bert_attention keeps one log-sum-exp per query row)")
    if config.hidden_act not in _ACTS:
        raise ValueError(f"BertModel: hidden_act {config.hidden_act!r} is not supported (one of {_ACTS})")
    if getattr(config, "pruned_heads", None):
        raise ValueError("BertModel: pruned_heads is not supported")


def checkpoint_key(key: str) -> str:
    """The state_dict name of a checkpoint tensor: checkpoints of models with heads carry the encoder under `bert.`, and
    TensorFlow-era ones call a LayerNorm's two vectors `gamma` and `beta`."""
    if key.startswith("bert."):
        key = key[len("bert."):]
    owner, dot, leaf = key.rpartition(".")
    return owner + dot + {"gamma": "weight", "beta": "bias"}.get(leaf, leaf)


# The dropout sites draw their seeds from ops.new_dropout_seed() in forward order: the embeddings, then per layer the attention
# probabilities, the attention output and the layer output.  A site draws only in training mode and with its p > 0.
def _drop(module: nn.Module, x, p: float, seeds: list):
    if not module.training or p <= 0:
        return x
    seed = ops.new_dropout_seed()
    seeds.append(seed)
    return ops.feat_dropout(x, p, seed)


class BertEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, padding_idx=0)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, input_ids, token_type_ids=None, position_ids=None, seeds=None):
        y = ops.bert_embed(self.word_embeddings.weight, self.position_embeddings.weight, self.token_type_embeddings.weight, input_ids,
                           position_ids, token_type_ids, self.LayerNorm.weight, self.LayerNorm.bias, self.LayerNorm.eps)
        return _drop(self, y, self.dropout.p, [] if seeds is None else seeds)


class BertSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = config.hidden_size // config.num_attention_heads
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        self.query = nn.Linear(config.hidden_size, self.all_head_size)
        self.key = nn.Linear(config.hidden_size, self.all_head_size)
        self.value = nn.Linear(config.hidden_size, self.all_head_size)
        self.dropout = nn.Dropout(config.attention_probs_dropout_prob)

    def forward(self, hidden_states, bias, seeds=None):
        q = ops.linear(hidden_states, self.query.weight, self.query.bias)
        k = ops.linear(hidden_states, self.key.weight, self.key.bias)
        v = ops.linear(hidden_states, self.value.weight, self.value.bias)
        p, seed = 0.0, 0
        if self.training and self.dropout.p > 0:
            p, seed = self.dropout.p, ops.new_dropout_seed()
            if seeds is not None:
                seeds.append(seed)
        return ops.bert_attention(q, k, v, bias, self.num_attention_heads, 1.0 / math.sqrt(self.attention_head_size), p, seed)


class _DenseDropNorm(nn.Module):
    """BertSelfOutput / BertOutput: LayerNorm(dropout(dense(hidden_states)) + input_tensor)."""

    def __init__(self, in_features, config):
        super().__init__()
        self.dense = nn.Linear(in_features, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, hidden_states, input_tensor, seeds=None):
        h = ops.linear(hidden_states, self.dense.weight, self.dense.bias)
        h = _drop(self, h, self.dropout.p, [] if seeds is None else seeds)
        return ops.add_layernorm(h, input_tensor, self.LayerNorm.weight, self.LayerNorm.bias, self.LayerNorm.eps)


class BertSelfOutput(_DenseDropNorm):
    def __init__(self, config):
        super().__init__(config.hidden_size, config)


class BertOutput(_DenseDropNorm):
    def __init__(self, config):
        super().__init__(config.intermediate_size, config)


class BertAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = BertSelfAttention(config)
        self.output = BertSelfOutput(config)

    def forward(self, input_tensor, bias, seeds=None):
        return self.output(self.self(input_tensor, bias, seeds), input_tensor, seeds)


class BertIntermediate(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)
        self.hidden_act = config.hidden_act

    def forward(self, hidden_states):
        h = ops.linear(hidden_states, self.dense.weight, self.dense.bias)
        return ops.gelu(h) if self.hidden_act == "gelu" else ops.relu(h)


class BertLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = BertAttention(config)
        self.intermediate = BertIntermediate(config)
        self.output = BertOutput(config)

    def forward(self, hidden_states, bias, seeds=None):
        attention_output = self.attention(hidden_states, bias, seeds)
        return self.output(self.intermediate(attention_output), attention_output, seeds)


class BertEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(config.num_hidden_layers)])

    def forward(self, hidden_states, bias, output_hidden_states=False, seeds=None):
        """-> (last hidden state,) or (last hidden state, (input, every layer's output))."""
        states = [hidden_states]
        for layer_module in self.layer:
            states.append(layer_module(states[-1], bias, seeds))
        return (states[-1], tuple(states)) if output_hidden_states else (states[-1],)


class BertPooler(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)

    def forward(self, hidden_states):
        return ops.tanh_act(ops.linear(hidden_states[:, 0], self.dense.weight, self.dense.bias))


class BertModel(nn.Module):
    """modeling_bert.py:532-628.  forward(input_ids, token_type_ids=None, attention_mask=None, position_ids=None,
    head_mask=None) -> (sequence_output (B,L,H), pooled_output (B,H)[, all hidden states]).  Ids are int32 or int64;
    attention_mask (B,L) of any dtype enters as the additive bias (1 - mask) * -10000, so a sequence that is all padding attends
    by its raw scores, as in the reference.  After a training-mode forward ``last_dropout_seeds`` lists the seeds drawn."""

    def __init__(self, config):
        super().__init__()
        if not isinstance(config, BertConfig):
            raise ValueError(f"BertModel: config must be a get_amd.bert.BertConfig, got {type(config).__name__} "
                             "(a saved model is built by BertModel.from_pretrained(directory))")
        _check_config(config)
        self.config = config
        self.register_load_state_dict_post_hook(lambda m, incompatible_keys: ops.bump_weight_epoch())
        self.embeddings = BertEmbeddings(config)
        self.encoder = BertEncoder(config)
        self.pooler = BertPooler(config)
        self.last_dropout_seeds = []
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self):
        """By parameter name (tests/golden/bert_contract.json lists them): LayerNorm weight 1 and bias 0, every other bias 0, every
        matrix and table normal(0, initializer_range) -- the word table's padding row included, as the reference draws it."""
        for name, p in self.named_parameters():
            if ".LayerNorm." in name:
                (nn.init.ones_ if name.endswith("weight") else nn.init.zeros_)(p)
            elif name.endswith(".bias"):
                nn.init.zeros_(p)
            else:
                nn.init.normal_(p, 0.0, self.config.initializer_range)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, position_ids=None, head_mask=None):
        config = self.config
        if head_mask is not None:
            raise ValueError("BertModel: head_mask is not supported: the attention probabilities are never materialised")
        _check_config(config)
        if input_ids.dim() != 2:
            raise ValueError(f"BertModel: input_ids (B,L) is expected, got {tuple(input_ids.shape)}")
        if input_ids.shape[1] > config.max_position_embeddings:
            raise ValueError(f"BertModel: sequence length {input_ids.shape[1]} exceeds max_position_embeddings "
                             f"{config.max_position_embeddings}")
        _lib.require_cuda(input_ids, token_type_ids, attention_mask, position_ids)
        bias = None
        if attention_mask is not None:      # modeling_bert.py:602-603, non-binary masks included
            bias = (1.0 - attention_mask.to(torch.float32)) * -10000.0
        seeds = []
        hidden = self.embeddings(input_ids, token_type_ids, position_ids, seeds)
        encoder_outputs = self.encoder(hidden, bias, config.output_hidden_states, seeds)
        sequence_output = encoder_outputs[0]
        self.last_dropout_seeds = seeds
        return (sequence_output, self.pooler(sequence_output)) + encoder_outputs[1:]

    def save_pretrained(self, directory):
        """Writes <directory>/config.json and <directory>/pytorch_model.bin, what from_pretrained reads."""
        self.config.save_pretrained(directory)
        torch.save(self.state_dict(), os.path.join(directory, WEIGHTS_NAME))

    @classmethod
    def from_pretrained(cls, directory):
        """The model of a local directory holding config.json and pytorch_model.bin, in evaluation mode as the reference's
        from_pretrained leaves it.  Keys are renamed by checkpoint_key (the reference's two rules, modeling_utils.py:339-350, :374).  Keys of other heads (`cls.*`) are ignored; a
        key the model has and the file lacks keeps its random initialisation, with a warning."""
        if not isinstance(directory, (str, os.PathLike)) or not os.path.isdir(directory):
            raise ValueError(f"BertModel.from_pretrained: {directory!r} is not a directory. Nothing is ever downloaded: pass a "
                             f"directory that holds {CONFIG_NAME} and {WEIGHTS_NAME}")
        for name in (CONFIG_NAME, WEIGHTS_NAME):
            if not os.path.isfile(os.path.join(directory, name)):
                raise ValueError(f"BertModel.from_pretrained: {os.path.join(directory, name)} is missing")
        model = cls(BertConfig.from_json_file(os.path.join(directory, CONFIG_NAME)))
        state = torch.load(os.path.join(directory, WEIGHTS_NAME), map_location="cpu", weights_only=True)
        renamed = {checkpoint_key(k): v for k, v in state.items()}
        own = model.state_dict()
        missing = [k for k in own if k not in renamed]
        if missing:
            warnings.warn(f"BertModel.from_pretrained: {directory} has no tensor for {missing}; they keep their random initialisation")
        model.load_state_dict({k: v for k, v in renamed.items() if k in own}, strict=False)
        return model.eval()


class BertModule(nn.Module):
    """matchzoo/modules/bert_module.py: ``bert`` applied to the concatenation of the two id tensors.  `mode` is a directory
    holding config.json and pytorch_model.bin (the layout the reference's from_pretrained reads), whose encoder is left in eval
    mode as from_pretrained leaves it, or a BertConfig for a randomly initialised encoder, which is for training and stays in
    training mode.  A model name is refused: nothing is ever downloaded."""

    def __init__(self, mode="bert-base-uncased"):
        super().__init__()
        if isinstance(mode, BertConfig):
            self.bert = BertModel(mode)
        elif isinstance(mode, (str, os.PathLike)) and os.path.isdir(mode):
            self.bert = BertModel.from_pretrained(mode)
        else:
            raise ValueError(f"BertModule: {mode!r} is neither a directory nor a BertConfig. Nothing is ever downloaded, so a "
                             f"model name cannot be served: a directory holding {CONFIG_NAME} and {WEIGHTS_NAME} is required")

    def forward(self, x, y):
        return self.bert(torch.cat((x, y), dim=-1))
