"""The word list of a closed-vocabulary benchmark (LRW: 500 words, LRW1000: 1000) as token rows, packed for
sbl_lexicon_shortlist (include/sbl_hip.h): Decoder.recognize_words maps the decoder's hypotheses onto it."""
import torch

from ._env import config, ops

MAX_WORD = ops.LEXICON_MAX_WORD          # tokens per word
MAX_WORDS = ops.LEXICON_MAX_WORDS


class Lexicon:
    """Wn >= 1 words; word w is a sequence of 1..15 token ids in [0, vocab), none of them sos or eos.  Duplicate rows are
    allowed and are distinct entries.

    words: a list of token-id sequences.  names: None, or one string per word (kept for reports; not used by the decode).
    device: where `packed` lives (default config.device).
    Attributes: tokens int64 (Wn, 15) CPU, IGNORE_ID behind the end; lengths int64 (Wn,) CPU; packed uint8 (Wn, 16) on
    `device`: bytes 0..14 the tokens (0 behind the end), byte 15 the length."""

    def __init__(self, words, names=None, device=None, vocab=config.vocab_size, sos_id=config.sos_id, eos_id=config.eos_id,
                 ignore_id=config.IGNORE_ID):
        words = [[int(t) for t in w] for w in words]
        if not 1 <= len(words) <= MAX_WORDS:
            raise ValueError("Lexicon: %d words (1..%d)" % (len(words), MAX_WORDS))
        if not 1 <= int(vocab) <= 64:
            raise ValueError("Lexicon: vocab = %d (the decode kernels hold one class per lane: 1..64)" % vocab)
        for i, w in enumerate(words):
            if not 1 <= len(w) <= MAX_WORD:
                raise ValueError("Lexicon: word %d has %d tokens (1..%d)" % (i, len(w), MAX_WORD))
            bad = [t for t in w if not 0 <= t < vocab or t in (sos_id, eos_id)]
            if bad:
                raise ValueError("Lexicon: word %d holds the id %d (ids are in [0, %d) and neither sos = %d nor eos = %d)"
                                 % (i, bad[0], vocab, sos_id, eos_id))
        if names is not None:
            names = [str(s) for s in names]
            if len(names) != len(words):
                raise ValueError("Lexicon: %d names for %d words" % (len(names), len(words)))
        self.names = names
        self.vocab, self.sos_id, self.eos_id, self.ignore_id = int(vocab), int(sos_id), int(eos_id), int(ignore_id)
        self.device = torch.device(config.device if device is None else device)
        self.lengths = torch.tensor([len(w) for w in words], dtype=torch.int64)
        self.tokens = torch.full((len(words), MAX_WORD), self.ignore_id, dtype=torch.int64)
        packed = torch.zeros(len(words), 16, dtype=torch.uint8)
        for i, w in enumerate(words):
            self.tokens[i, :len(w)] = torch.tensor(w, dtype=torch.int64)
            packed[i, :len(w)] = torch.tensor(w, dtype=torch.uint8)
        packed[:, 15] = self.lengths.to(torch.uint8)
        self.packed = packed.to(self.device)

    def __len__(self):
        return self.tokens.size(0)

    def word(self, w):
        """The token ids of word w as a list."""
        return self.tokens[w, :int(self.lengths[w])].tolist()

    @classmethod
    def from_targets(cls, gold, names=None, device=None, **ids):
        """A lexicon from IGNORE_ID-padded target rows gold (M, To), e.g. every label of a data set: the rows stripped of
        sos / eos / IGNORE_ID, deduplicated in first-occurrence order.  Returns (lexicon, index) with index int64 (M,) the
        word of every row: the `gold_word` of WordAccuracyMeter from the labels the caller already has."""
        sos, eos, ign = (ids.get(k, d) for k, d in (("sos_id", config.sos_id), ("eos_id", config.eos_id), ("ignore_id", config.IGNORE_ID)))
        seen, words, index = {}, [], []
        for row in torch.as_tensor(gold).cpu().tolist():
            w = tuple(t for t in row if t not in (sos, eos, ign))
            if w not in seen:
                seen[w] = len(words)
                words.append(list(w))
            index.append(seen[w])
        return cls(words, names=names, device=device, **ids), torch.tensor(index, dtype=torch.int64)
