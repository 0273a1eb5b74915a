#!/usr/bin/env python3
"""Writes tests/golden/nmt_nfkc_charsmap.bin: the precompiled character map of sentencepiece's `nmt_nfkc` normalisation rule (the rule
of XLM-R-style tokenizers), as sentencepiece stores it in a model it trains -- a u32 trie size, a darts-clone double array, a pool of
NUL-terminated strings.  The vocabulary trained on the way is thrown away.  Run: python tests/golden/make_charsmap.py"""
import io
import os
import random

import sentencepiece as spm
from sentencepiece import sentencepiece_model_pb2 as pb

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nmt_nfkc_charsmap.bin")


def main():
    rng = random.Random(7)
    words = ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(1, 8))) for _ in range(300)]
    lines = [" ".join(rng.choice(words) for _ in range(rng.randint(3, 12))) for _ in range(4000)]
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(lines), model_writer=model, model_type="unigram", normalization_rule_name="nmt_nfkc",
                                   vocab_size=90, hard_vocab_limit=False)
    m = pb.ModelProto()
    m.ParseFromString(model.getvalue())
    blob = m.normalizer_spec.precompiled_charsmap
    with open(OUT, "wb") as f:
        f.write(blob)
    print("wrote", OUT, len(blob), "bytes; trie", int.from_bytes(blob[:4], "little"))


if __name__ == "__main__":
    main()
