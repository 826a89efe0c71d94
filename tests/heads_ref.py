"""Float64 restatement of the BERT task heads and of their loss (tests only), on top of tests/bert_ref.py: the softmax
cross-entropy with an ignore index as include/get_hip.h states it (gh_softmax_xent_fwd / _bwd), the five head blocks and the
seven task models of pytorch_transformers/modeling_bert.py:377-442, :634-1148, written from the formulas in plain torch.  The GPU
tests compare the kernels and the drop-in classes with it (tests/test_gpu_loss_paths.py, tests/test_gpu_bert_heads.py);
tests/test_bert_heads_cpu.py checks it on its own against the reference's goldens and against torch's cross_entropy.

Edge semantics of the loss, pinned here: no kept row -> NaN loss (0 / 0) and a zero gradient; c = 1 -> loss 0, gradient 0; a
label outside [0, c) other than the ignore index (torch raises) -> the row is dropped like an ignored one."""
import torch

from tests import bert_ref


def kept_rows(labels, c, ignore_index):
    labels = labels.reshape(-1).long()
    return (labels != ignore_index) & (labels >= 0) & (labels < c)


def xent(x, labels, ignore_index=-100):
    """x (rows, c) float64, labels (rows,) -> (loss scalar, lse (rows,), n_kept); differentiable in x."""
    rows, c = x.shape
    labels = labels.reshape(-1).long()
    kept = kept_rows(labels, c, ignore_index)
    lse = torch.logsumexp(x, dim=1)
    picked = x.gather(1, labels.clamp(0, c - 1).unsqueeze(1)).squeeze(1)
    row_loss = torch.where(kept, lse - picked, torch.zeros_like(lse))
    n = int(kept.sum())
    return row_loss.sum() / torch.tensor(float(n), dtype=x.dtype), lse, n


def xent_grad(x, labels, lse, n_kept, g, ignore_index=-100):
    """dx (rows, c) = (exp(x - lse) - onehot(label)) g / n_kept on the kept rows, exact zeros elsewhere."""
    rows, c = x.shape
    labels = labels.reshape(-1).long()
    kept = kept_rows(labels, c, ignore_index)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(rows)[kept], labels[kept]] = 1.0
    dx = (torch.exp(x - lse.unsqueeze(1)) - onehot) * (g / max(n_kept, 1))
    return torch.where(kept.unsqueeze(1), dx, torch.zeros_like(dx))


def loss_of(logits, labels, ignore_index=-100):
    """The loss of logits (..., c) and labels of the leading shape, as the task models call it."""
    return xent(logits.reshape(-1, logits.shape[-1]), labels, ignore_index)[0]


# ----------------------------------------------------------------------------- heads
def transform(p, prefix, x, eps, act="gelu"):
    h = bert_ref.linear(p, prefix + "dense", x)
    h = bert_ref.gelu(h) if act == "gelu" else torch.relu(h)
    return bert_ref.layer_norm(h, p[prefix + "LayerNorm.weight"], p[prefix + "LayerNorm.bias"], eps)


def lm_head(p, x, config):
    """cls.predictions: decoder(transform(x)) + bias, the decoder's weight being the word table."""
    h = transform(p, "cls.predictions.transform.", x, config["layer_norm_eps"], config["hidden_act"])
    return h @ p["cls.predictions.decoder.weight"].t() + p["cls.predictions.bias"]


def _encoder(p, config, ids, types, mask, masks=None):
    """bert.* of a task model through tests/bert_ref.py -> (sequence_output, pooled_output)."""
    enc = {k[len("bert."):]: v for k, v in p.items() if k.startswith("bert.")}
    seq, pooled, _ = bert_ref.model(enc, config, ids, types, mask, masks=masks)
    return seq, pooled


def task_model(cls, p, config, inputs, masks=None, head_keep=None):
    """The forward of the task model named `cls` in float64: p = parameters by state_dict name (tied names hold one tensor),
    inputs = the forward's keyword arguments -> the reference's output tuple (loss first when the labels are given).
    masks: the encoder's dropout keep masks (bert_ref.model); head_keep: the keep mask of the head's own dropout."""
    ids, types, mask = inputs["input_ids"], inputs.get("token_type_ids"), inputs.get("attention_mask")
    p_h = config["hidden_dropout_prob"]
    if cls == "BertForMultipleChoice":
        flat = lambda t: t.reshape(-1, t.shape[-1]) if t is not None else None
        seq, pooled = _encoder(p, config, flat(ids), flat(types), flat(mask), masks)
    else:
        seq, pooled = _encoder(p, config, ids, types, mask, masks)
    if cls == "BertForPreTraining":
        scores, rel = lm_head(p, seq, config), bert_ref.linear(p, "cls.seq_relationship", pooled)
        out = (scores, rel)
        if inputs.get("masked_lm_labels") is not None and inputs.get("next_sentence_label") is not None:
            out = (loss_of(scores, inputs["masked_lm_labels"], -1) + loss_of(rel, inputs["next_sentence_label"], -1),) + out
        return out
    if cls == "BertForMaskedLM":
        scores = lm_head(p, seq, config)
        labels = inputs.get("masked_lm_labels")
        return (scores,) if labels is None else (loss_of(scores, labels, -1), scores)
    if cls == "BertForNextSentencePrediction":
        rel = bert_ref.linear(p, "cls.seq_relationship", pooled)
        labels = inputs.get("next_sentence_label")
        return (rel,) if labels is None else (loss_of(rel, labels, -1), rel)
    if cls in ("BertForSequenceClassification", "BertForMultipleChoice"):
        logits = bert_ref.linear(p, "classifier", bert_ref.dropout(pooled, head_keep, p_h))
        if cls == "BertForMultipleChoice":
            logits = logits.reshape(-1, ids.shape[1])
        labels = inputs.get("labels")
        if labels is None:
            return (logits,)
        if cls == "BertForSequenceClassification" and logits.shape[-1] == 1:
            return (((logits.reshape(-1) - labels.reshape(-1).to(logits.dtype)) ** 2).mean(), logits)
        return (loss_of(logits, labels), logits)
    if cls == "BertForTokenClassification":
        logits = bert_ref.linear(p, "classifier", bert_ref.dropout(seq, head_keep, p_h))
        labels = inputs.get("labels")
        if labels is None:
            return (logits,)
        flat = labels.reshape(-1)
        if mask is not None:
            flat = torch.where(mask.reshape(-1) == 1, flat, torch.full_like(flat, -100))
        return (loss_of(logits, flat), logits)
    if cls == "BertForQuestionAnswering":
        logits = bert_ref.linear(p, "qa_outputs", seq)
        start, end = logits[..., 0], logits[..., 1]
        sp, ep = inputs.get("start_positions"), inputs.get("end_positions")
        if sp is None or ep is None:
            return (start, end)
        L = start.shape[1]
        squeeze = lambda t: t.squeeze(-1) if t.dim() > 1 else t
        loss = (loss_of(start, squeeze(sp).clamp(0, L), L) + loss_of(end, squeeze(ep).clamp(0, L), L)) / 2
        return (loss, start, end)
    raise ValueError(cls)
