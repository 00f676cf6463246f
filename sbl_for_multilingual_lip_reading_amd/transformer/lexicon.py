"""The word list of a closed-vocabulary benchmark (LRW: 500 words, LRW1000: 1000) as token rows, packed for
sbl_lexicon_shortlist (include/sbl_hip.h): Decoder.recognize_words maps the decoder's hypotheses onto it.  Its trie
(Lexicon.trie) constrains the beam search of the single-direction model (Seq2SeqDecoder.recognize_words, sbl_beam_tail_lex),
its trie over pairs of tokens (Lexicon.pair_trie) the pair beam search of the SBL decoder (Decoder.beam_search_lex,
sbl_pair_beam_tail_lex)."""
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
        self.max_len = int(self.lengths.max())
        self._trie = None
        self._pair_trie = None

    def __len__(self):
        return self.tokens.size(0)

    def word(self, w):
        """The token ids of word w as a list."""
        return self.tokens[w, :int(self.lengths[w])].tolist()

    def trie(self):
        """The (mask int64, first int32, word int32) tables of the lexicon's trie on `device`, each of P entries, as
        include/sbl_hip.h defines them (node 0 the empty prefix, breadth-first numbering with siblings in ascending token
        id; bit v of mask[p]: prefix(p) + [v] is a node, bit eos: prefix(p) is a word; first[p] the lowest-token child, 0
        at a leaf; word[p] the lowest word index that spells prefix(p) or -1).  Built once on the host and cached."""
        if self._trie is None:
            kids, owner = [{}], [-1]          # insertion-numbered first, then renumbered breadth-first
            for i, (row, c) in enumerate(zip(self.tokens.tolist(), self.lengths.tolist())):
                p = 0
                for t in row[:c]:
                    if t not in kids[p]:
                        kids[p][t] = len(kids)
                        kids.append({})
                        owner.append(-1)
                    p = kids[p][t]
                if owner[p] < 0:
                    owner[p] = i
            order = [0]
            for p in order:                   # grows while it is walked: a queue
                order.extend(kids[p][t] for t in sorted(kids[p]))
            new = {old: k for k, old in enumerate(order)}
            mask, first, word = [], [], []
            for old in order:
                bits = sum(1 << t for t in kids[old]) | ((1 << self.eos_id) if owner[old] >= 0 else 0)
                mask.append(bits - (1 << 64) if bits >> 63 else bits)      # the bit pattern as a signed 64-bit value
                first.append(new[kids[old][min(kids[old])]] if kids[old] else 0)
                word.append(owner[old])
            self._trie = (torch.tensor(mask, dtype=torch.int64).to(self.device), torch.tensor(first, dtype=torch.int32).to(self.device),
                          torch.tensor(word, dtype=torch.int32).to(self.device))
        return self._trie

    def pair_trie(self):
        """The (begin int32 (P + 1), key int32 (P - 1), word int32 (P)) tables of the lexicon's PAIR trie on `device`, as
        include/sbl_hip.h defines them for sbl_pair_beam_tail_lex (Decoder.beam_search_lex).  A node is what both directions
        have emitted after t steps of one word of c tokens, (w[:t], w[c-t:]); node 0 the empty state; one terminal node per
        distinct word behind the key (eos, eos) of its depth-c state.  Edge key = a * 64 + b with (a, b) = (w[t], w[c-1-t]);
        breadth-first numbering with the children of a node in ascending key, so the child behind CSR entry e is node e + 1.
        word[p]: at a terminal node the lowest word index that spells it, -1 elsewhere.  Built once on the host and cached."""
        if self._pair_trie is None:
            kids, owner = [{}], [-1]          # insertion-numbered first, then renumbered breadth-first
            for i, (row, c) in enumerate(zip(self.tokens.tolist(), self.lengths.tolist())):
                w = row[:c]
                p = 0
                for k in [w[t] * 64 + w[c - 1 - t] for t in range(c)] + [self.eos_id * 64 + self.eos_id]:
                    if k not in kids[p]:
                        kids[p][k] = len(kids)
                        kids.append({})
                        owner.append(-1)
                    p = kids[p][k]
                if owner[p] < 0:
                    owner[p] = i
            order = [0]
            for p in order:                   # grows while it is walked: a queue
                order.extend(kids[p][k] for k in sorted(kids[p]))
            begin, key, word = [0], [], []
            for old in order:
                key.extend(sorted(kids[old]))
                begin.append(len(key))
                word.append(owner[old])
            self._pair_trie = tuple(torch.tensor(t, dtype=torch.int32).to(self.device) for t in (begin, key, word))
        return self._pair_trie

    def lookup(self, ys):
        """The word index of every token row of ys int64 (..., Ly) on `device` (rows as recognize / beam_search return them:
        entry 0 is skipped, the row is cut before the first eos, sos / ignore entries are dropped), -1 where the tokens spell
        no word: int32 of shape ys.shape[:-1].  Duplicate words answer with their lowest index.  One launch
        (sbl_lexicon_lookup), no sync."""
        return ops.lexicon_lookup(ys, self.trie(), self.sos_id, self.eos_id, self.ignore_id)[0]

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
