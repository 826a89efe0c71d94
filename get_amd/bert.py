"""The BERT encoder as a drop-in: ``BertConfig``, ``BertModel`` (pytorch_transformers/modeling_bert.py:142-375, 532-631) and
``BertModule`` (matchzoo/modules/bert_module.py:9-30), backed by csrc/bert_ops.hip and the project's linear, LayerNorm,
embedding and dropout kernels.

``BertModel`` has the reference's module tree, so a reference checkpoint loads unchanged: 5 + 16 * layers + 2 state_dict
keys under ``embeddings.*``, ``encoder.layer.N.*`` and ``pooler.dense.*``.  The attention probabilities are never materialised
(ops.bert_attention), which is why ``output_attentions`` and ``head_mask`` are refused.  Nothing is ever downloaded: a
pretrained model is a local directory holding ``config.json`` and ``pytorch_model.bin``.

The task heads (modeling_bert.py:377-442) and the seven task models (:634-1148, ``TASK_MODELS``) sit on top of it under the
reference's names, signatures, return tuples and state_dict keys; their losses are ops.softmax_cross_entropy
(csrc/loss_ops.hip), and the masked-LM decoder's weight is the word table's Parameter.
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


def _leaf_key(key: str) -> str:
    """A checkpoint tensor's name with the TensorFlow-era `gamma` / `beta` of a LayerNorm renamed (modeling_utils.py:339-350)."""
    owner, dot, leaf = key.rpartition(".")
    return owner + dot + {"gamma": "weight", "beta": "bias"}.get(leaf, leaf)


def checkpoint_key(key: str) -> str:
    """The state_dict name of a checkpoint tensor: checkpoints of models with heads carry the encoder under `bert.`, and
    TensorFlow-era ones call a LayerNorm's two vectors `gamma` and `beta`."""
    return _leaf_key(key[len("bert."):] if key.startswith("bert.") else key)


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


# ----------------------------------------------------------------------------- the task heads (modeling_bert.py:377-442)
class BertPredictionHeadTransform(nn.Module):
    """:377-391: LayerNorm(act(dense(hidden_states)))."""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.hidden_act = config.hidden_act
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def forward(self, hidden_states):
        h = ops.linear(hidden_states, self.dense.weight, self.dense.bias)
        h = ops.gelu(h) if self.hidden_act == "gelu" else ops.relu(h)
        return ops.add_layernorm(h, None, self.LayerNorm.weight, self.LayerNorm.bias, self.LayerNorm.eps)


class BertLMPredictionHead(nn.Module):
    """:394-410: decoder(transform(hidden_states)) + bias, (.., vocab_size).  The decoder's weight is the word table once the
    owning model has tied it."""

    def __init__(self, config):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.bias = nn.Parameter(torch.zeros(config.vocab_size))

    def forward(self, hidden_states):
        return ops.linear(self.transform(hidden_states), self.decoder.weight, self.bias)


class BertOnlyMLMHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.predictions = BertLMPredictionHead(config)

    def forward(self, sequence_output):
        return self.predictions(sequence_output)


class BertOnlyNSPHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.seq_relationship = nn.Linear(config.hidden_size, 2)

    def forward(self, pooled_output):
        return ops.linear(pooled_output, self.seq_relationship.weight, self.seq_relationship.bias)


class BertPreTrainingHeads(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.predictions = BertLMPredictionHead(config)
        self.seq_relationship = nn.Linear(config.hidden_size, 2)

    def forward(self, sequence_output, pooled_output):
        return self.predictions(sequence_output), ops.linear(pooled_output, self.seq_relationship.weight, self.seq_relationship.bias)


TIED_KEYS = ("cls.predictions.decoder.weight", "bert.embeddings.word_embeddings.weight")


class _BertTaskModel(nn.Module):
    """What the seven task models share: the encoder under ``bert``, the heads' initialisation (modeling_bert.py:456-467), the
    tie of the decoder to the word table, and the local-directory from_pretrained / save_pretrained."""

    def __init__(self, config):
        super().__init__()
        if not isinstance(config, BertConfig):
            raise ValueError(f"{type(self).__name__}: config must be a get_amd.bert.BertConfig, got {type(config).__name__} "
                             f"(a saved model is built by {type(self).__name__}.from_pretrained(directory))")
        self.config = config
        self.register_load_state_dict_post_hook(lambda m, incompatible_keys: (m.tie_weights(), ops.bump_weight_epoch()) and None)
        self.bert = BertModel(config)

    @property
    def last_dropout_seeds(self):
        """The seeds the last training-mode forward drew, the encoder's first and then the head's, in forward order."""
        return self.bert.last_dropout_seeds

    def tie_weights(self):
        """:680-685, :748-753: the decoder's weight IS the word table (one Parameter under two state_dict keys)."""
        cls = getattr(self, "cls", None)
        if cls is not None and hasattr(cls, "predictions"):
            cls.predictions.decoder.weight = self.bert.embeddings.word_embeddings.weight

    @torch.no_grad()
    def _init_heads(self):
        self.tie_weights()
        for name, p in self.named_parameters():
            if name.startswith("bert."):
                continue
            if ".LayerNorm." in name:
                (nn.init.ones_ if name.endswith("weight") else nn.init.zeros_)(p)
            elif name.endswith("bias"):
                nn.init.zeros_(p)
            else:
                nn.init.normal_(p, 0.0, self.config.initializer_range)

    def _encode(self, input_ids, token_type_ids, attention_mask, position_ids, head_mask):
        return self.bert(input_ids, token_type_ids=token_type_ids, attention_mask=attention_mask, position_ids=position_ids,
                         head_mask=head_mask)

    def _head_drop(self, x):
        """The head's own dropout (:868, :972, :1040); its seed follows the encoder's in last_dropout_seeds."""
        return _drop(self, x, self.dropout.p, self.bert.last_dropout_seeds)

    def save_pretrained(self, directory):
        """Writes <directory>/config.json and <directory>/pytorch_model.bin, what from_pretrained reads."""
        self.config.save_pretrained(directory)
        torch.save(self.state_dict(), os.path.join(directory, WEIGHTS_NAME))

    @classmethod
    def from_pretrained(cls, directory):
        """The model of a local directory holding config.json and pytorch_model.bin, in evaluation mode.  The file's keys either
        carry the encoder under `bert.` (a checkpoint of any task model: its heads are read too) or are a bare BertModel's, which
        then fills the encoder alone (modeling_utils.py:372-379); `gamma` / `beta` are renamed.  A tensor the model has and the
        file lacks keeps its initialisation, with a warning; the decoder is tied to the word table again."""
        name = cls.__name__
        if not isinstance(directory, (str, os.PathLike)) or not os.path.isdir(directory):
            raise ValueError(f"{name}.from_pretrained: {directory!r} is not a directory. Nothing is ever downloaded: pass a "
                             f"directory that holds {CONFIG_NAME} and {WEIGHTS_NAME}")
        for f in (CONFIG_NAME, WEIGHTS_NAME):
            if not os.path.isfile(os.path.join(directory, f)):
                raise ValueError(f"{name}.from_pretrained: {os.path.join(directory, f)} is missing")
        model = cls(BertConfig.from_json_file(os.path.join(directory, CONFIG_NAME)))
        state = torch.load(os.path.join(directory, WEIGHTS_NAME), map_location="cpu", weights_only=True)
        prefixed = any(k.startswith("bert.") for k in state)
        renamed = {(_leaf_key(k) if prefixed else "bert." + _leaf_key(k)): v for k, v in state.items()}
        own = model.state_dict()
        tied = set(TIED_KEYS) if TIED_KEYS[0] in own else set()
        missing = [k for k in own if k not in renamed and not (k in tied and tied & set(renamed))]
        if missing:
            warnings.warn(f"{name}.from_pretrained: {directory} has no tensor for {missing}; they keep their random initialisation")
        model.load_state_dict({k: v for k, v in renamed.items() if k in own}, strict=False)
        model.tie_weights()
        return model.eval()


def _flat_labels(labels, what, rows):
    if labels.numel() != rows:
        raise ValueError(f"{what}: {labels.numel()} labels for {rows} rows of logits")
    return labels.reshape(-1)


class BertForPreTraining(_BertTaskModel):
    """:634-704.  forward(input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None, next_sentence_label=None,
    position_ids=None, head_mask=None) -> ((loss,) prediction_scores (B,L,V), seq_relationship_score (B,2)[, hidden states]);
    the loss, with both label tensors given, is the sum of the two cross-entropies, labels of -1 ignored."""

    def __init__(self, config):
        super().__init__(config)
        self.cls = BertPreTrainingHeads(config)
        self._init_heads()

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None, next_sentence_label=None,
                position_ids=None, head_mask=None):
        outputs = self._encode(input_ids, token_type_ids, attention_mask, position_ids, head_mask)
        prediction_scores, seq_relationship_score = self.cls(outputs[0], outputs[1])
        outputs = (prediction_scores, seq_relationship_score) + outputs[2:]
        if masked_lm_labels is not None and next_sentence_label is not None:
            _lib.require_cuda(masked_lm_labels, next_sentence_label)
            masked_lm_loss = ops.softmax_cross_entropy(prediction_scores, masked_lm_labels, ignore_index=-1)
            next_sentence_loss = ops.softmax_cross_entropy(seq_relationship_score, next_sentence_label.reshape(-1), ignore_index=-1)
            outputs = (masked_lm_loss + next_sentence_loss,) + outputs
        return outputs


class BertForMaskedLM(_BertTaskModel):
    """:709-769.  forward(input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None, position_ids=None,
    head_mask=None) -> ((masked_lm_loss,) prediction_scores (B,L,V)[, hidden states]); labels of -1 are ignored."""

    def __init__(self, config):
        super().__init__(config)
        self.cls = BertOnlyMLMHead(config)
        self._init_heads()

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None, position_ids=None, head_mask=None):
        outputs = self._encode(input_ids, token_type_ids, attention_mask, position_ids, head_mask)
        prediction_scores = self.cls(outputs[0])
        outputs = (prediction_scores,) + outputs[2:]
        if masked_lm_labels is not None:
            _lib.require_cuda(masked_lm_labels)
            outputs = (ops.softmax_cross_entropy(prediction_scores, masked_lm_labels, ignore_index=-1),) + outputs
        return outputs


class BertForNextSentencePrediction(_BertTaskModel):
    """:774-826.  forward(input_ids, token_type_ids=None, attention_mask=None, next_sentence_label=None, position_ids=None,
    head_mask=None) -> ((next_sentence_loss,) seq_relationship_score (B,2)[, hidden states]); labels of -1 are ignored."""

    def __init__(self, config):
        super().__init__(config)
        self.cls = BertOnlyNSPHead(config)
        self._init_heads()

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, next_sentence_label=None, position_ids=None, head_mask=None):
        outputs = self._encode(input_ids, token_type_ids, attention_mask, position_ids, head_mask)
        seq_relationship_score = self.cls(outputs[1])
        outputs = (seq_relationship_score,) + outputs[2:]
        if next_sentence_label is not None:
            _lib.require_cuda(next_sentence_label)
            outputs = (ops.softmax_cross_entropy(seq_relationship_score, next_sentence_label.reshape(-1), ignore_index=-1),) + outputs
        return outputs


class BertForSequenceClassification(_BertTaskModel):
    """:832-894.  forward(input_ids, token_type_ids=None, attention_mask=None, labels=None, position_ids=None, head_mask=None)
    -> ((loss,) logits (B,num_labels)[, hidden states]).  config.num_labels == 1 is a regression: the mean squared error (B
    values, plain tensor arithmetic); otherwise the cross-entropy."""

    def __init__(self, config):
        super().__init__(config)
        self.num_labels = config.num_labels
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.classifier = nn.Linear(config.hidden_size, config.num_labels)
        self._init_heads()

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, labels=None, position_ids=None, head_mask=None):
        outputs = self._encode(input_ids, token_type_ids, attention_mask, position_ids, head_mask)
        logits = ops.linear(self._head_drop(outputs[1]), self.classifier.weight, self.classifier.bias)
        outputs = (logits,) + outputs[2:]
        if labels is not None:
            _lib.require_cuda(labels)
            if self.num_labels == 1:
                loss = ((logits.view(-1) - labels.view(-1).to(logits.dtype)) ** 2).mean()
            else:
                loss = ops.softmax_cross_entropy(logits, _flat_labels(labels, "BertForSequenceClassification", logits.shape[0]))
            outputs = (loss,) + outputs
        return outputs


class BertForMultipleChoice(_BertTaskModel):
    """:900-1000.  forward(input_ids (B,C,L), token_type_ids=None, attention_mask=None, labels=None (B,), position_ids=None,
    head_mask=None) -> ((loss,) reshaped_logits (B,C)[, hidden states]): every choice is encoded as a sequence of its own."""

    def __init__(self, config):
        super().__init__(config)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.classifier = nn.Linear(config.hidden_size, 1)
        self._init_heads()

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, labels=None, position_ids=None, head_mask=None):
        if input_ids.dim() != 3:
            raise ValueError(f"BertForMultipleChoice: input_ids (B,num_choices,L) is expected, got {tuple(input_ids.shape)}")
        num_choices = input_ids.shape[1]
        flat = lambda t: t.reshape(-1, t.shape[-1]) if t is not None else None
        outputs = self._encode(flat(input_ids), flat(token_type_ids), flat(attention_mask), flat(position_ids), head_mask)
        logits = ops.linear(self._head_drop(outputs[1]), self.classifier.weight, self.classifier.bias)
        reshaped_logits = logits.view(-1, num_choices)
        outputs = (reshaped_logits,) + outputs[2:]
        if labels is not None:
            _lib.require_cuda(labels)
            loss = ops.softmax_cross_entropy(reshaped_logits, _flat_labels(labels, "BertForMultipleChoice", reshaped_logits.shape[0]))
            outputs = (loss,) + outputs
        return outputs


class BertForTokenClassification(_BertTaskModel):
    """:1006-1067.  forward(input_ids, token_type_ids=None, attention_mask=None, labels=None (B,L), position_ids=None,
    head_mask=None) -> ((loss,) scores (B,L,num_labels)[, hidden states]).  With a mask the loss keeps the tokens whose mask is 1
    (:1059): the other tokens' labels become the ignore index, which gathers nothing and never waits for the device."""

    def __init__(self, config):
        super().__init__(config)
        self.num_labels = config.num_labels
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.classifier = nn.Linear(config.hidden_size, config.num_labels)
        self._init_heads()

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, labels=None, position_ids=None, head_mask=None):
        outputs = self._encode(input_ids, token_type_ids, attention_mask, position_ids, head_mask)
        logits = ops.linear(self._head_drop(outputs[0]), self.classifier.weight, self.classifier.bias)
        outputs = (logits,) + outputs[2:]
        if labels is not None:
            _lib.require_cuda(labels)
            flat = _flat_labels(labels, "BertForTokenClassification", logits.shape[0] * logits.shape[1])
            if attention_mask is not None:
                flat = torch.where(attention_mask.reshape(-1) == 1, flat, torch.full_like(flat, -100))
            outputs = (ops.softmax_cross_entropy(logits, flat.view(logits.shape[:-1])),) + outputs
        return outputs


class BertForQuestionAnswering(_BertTaskModel):
    """:1073-1148.  forward(input_ids, token_type_ids=None, attention_mask=None, start_positions=None, end_positions=None,
    position_ids=None, head_mask=None) -> ((loss,) start_logits (B,L), end_logits (B,L)[, hidden states]).  The two logit
    tensors are the columns of one (B,L,2) tensor and both losses read them there.  Positions are clamped to [0, L] and L is
    the ignore index (:1138-1142); the caller's position tensors are left as they are (the reference clamps them in place)."""

    def __init__(self, config):
        super().__init__(config)
        self.num_labels = config.num_labels
        self.qa_outputs = nn.Linear(config.hidden_size, config.num_labels)
        self._init_heads()

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, start_positions=None, end_positions=None,
                position_ids=None, head_mask=None):
        outputs = self._encode(input_ids, token_type_ids, attention_mask, position_ids, head_mask)
        logits = ops.linear(outputs[0], self.qa_outputs.weight, self.qa_outputs.bias)
        if logits.shape[-1] != 2:
            raise ValueError(f"BertForQuestionAnswering: config.num_labels must be 2 (start, end), got {logits.shape[-1]}")
        start_logits, end_logits = logits[..., 0], logits[..., 1]
        outputs = (start_logits, end_logits) + outputs[2:]
        if start_positions is not None and end_positions is not None:
            _lib.require_cuda(start_positions, end_positions)
            ignored_index = start_logits.shape[1]
            losses = []
            for lg, pos in ((start_logits, start_positions), (end_logits, end_positions)):
                if pos.dim() > 1:
                    pos = pos.squeeze(-1)
                losses.append(ops.softmax_cross_entropy(lg, pos.clamp(0, ignored_index), ignore_index=ignored_index))
            outputs = ((losses[0] + losses[1]) / 2,) + outputs
        return outputs


TASK_MODELS = (BertForPreTraining, BertForMaskedLM, BertForNextSentencePrediction, BertForSequenceClassification,
               BertForMultipleChoice, BertForTokenClassification, BertForQuestionAnswering)


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
