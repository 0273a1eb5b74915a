"""Loading a real model2vec model directory (tokenizer.json + model.safetensors + config.json) for the host layer.

Tokenisation uses the Hugging Face `tokenizers` package -- the same Rust library the reference reaches through
model2vec-rs -- plugged into the C++ host layer as a callback tokenizer; the embedding table is uploaded once.
(The hub download of StaticModel::from_pretrained is out of scope: no network here.  Point this at a local copy
of minishlab/potion-multilingual-128M and the pipeline is the reference's: encode_batch(add_special_tokens=False)
-> drop unk -> truncate -> pool on the GPU.)"""
import json
import os

import numpy as np

from . import host


def read_model_tensors(model_dir):
    """(table as stored, uint32 mapping or None, float32 weights or None) of a model directory's model.safetensors.  `embeddings`
    keeps its dtype (F32 / F16 / I8).  A vocabulary-quantised model also carries `mapping` [n_tokens] (I32 / I64: token id -> table
    row; a negative entry is an error) and / or `weights` [n_tokens] (F64 / F32 / F16: one scalar per token, converted to float32 by
    value).  The tokenizer's vocabulary belongs to n_tokens then, not to the table's rows."""
    from safetensors.numpy import load_file

    from . import _lib as L

    tensors = load_file(os.path.join(model_dir, "model.safetensors"))
    table = np.ascontiguousarray(tensors["embeddings"])
    L.table_dtype_code(table.dtype)
    mapping, weights = tensors.get("mapping"), tensors.get("weights")
    if mapping is not None and mapping.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise TypeError(f"mapping dtype {mapping.dtype} is not supported (int32, int64)")
    if weights is not None and weights.dtype not in (np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(f"weights dtype {weights.dtype} is not supported (float64, float32, float16)")
    mapping, weights, _ = L.token_arrays(mapping, weights, table.shape[0])
    return table, mapping, weights


def load_static_model(ctx, model_dir):
    from tokenizers import Tokenizer

    tok = Tokenizer.from_file(os.path.join(model_dir, "tokenizer.json"))
    table, mapping, weights = read_model_tensors(model_dir)
    if mapping is not None or weights is not None:
        # (the callback-tokenizer creator takes a plain f32 table; the weights belong to the token, so nothing is remapped on the host)
        raise NotImplementedError("a vocabulary-quantised model (mapping / weights) is served by host.StaticModel(ctx, model_dir=...), "
                                  "which reads tokenizer.json natively")
    emb = np.ascontiguousarray(table.astype(np.float32))
    normalize = True
    cfg_path = os.path.join(model_dir, "config.json")
    if os.path.exists(cfg_path):
        normalize = bool(json.load(open(cfg_path)).get("normalize", True))
    spec = json.loads(tok.to_str())
    unk_token = (spec.get("model") or {}).get("unk_token")
    if unk_token is None and (spec.get("model") or {}).get("unk_id") is not None:      # Unigram stores an index
        unk_id = int(spec["model"]["unk_id"])
    else:
        unk_id = tok.token_to_id(unk_token) if unk_token else None
    vocab = tok.get_vocab()
    lens = sorted(len(t.encode("utf-8")) for t in vocab)                                   # model2vec: median of tk.len() -- BYTES
    median_len = max(1, lens[len(lens) // 2]) if lens else 5

    def encode(text):
        return tok.encode(text, add_special_tokens=False).ids

    return host.StaticModel(ctx, table=emb, tokenizer=encode, normalize=normalize, unk_id=unk_id, median_len=median_len)
