"""`clip.tokenize` (reference clip/clip.py:205-245): CLIP's byte-level BPE, written here from the published scheme.

A text is cleaned (`ftfy.fix_text` when ftfy is installed, HTML entities unescaped twice, whitespace runs collapsed,
stripped, lower-cased), split into words by the CLIP pre-tokenizer pattern, every word's UTF-8 bytes are mapped to 256
printable code points and merged by the ranked pair merges of the vocabulary file; the last symbol of a word carries the
end-of-word marker `</w>`.

Vocabulary ids: the 256 byte symbols, the same 256 with `</w>`, one id per merge (in rank order), then
`<|startoftext|>` and `<|endoftext|>`.  The merges file (`bpe_simple_vocab_16e6.txt.gz`, shipped with the reference CLIP)
is not part of this package: `set_bpe_path(path)` names it, or it is found in any directory of the `clip` package path
(`install_dropin(reference_root=...)` adds `<reference_root>/clip`).
"""
import gzip
import html
import os

import regex
import torch

BPE_NAME = "bpe_simple_vocab_16e6.txt.gz"
SOT, EOT = "<|startoftext|>", "<|endoftext|>"
N_MERGES = 49152 - 256 - 2              # merges of the CLIP vocabulary (49408 ids in all)
_WORDS = regex.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+",
                       regex.IGNORECASE)
_SPACES = regex.compile(r"\s+")

_bpe_path = None
_cache = {}


class BPENotFound(RuntimeError):
    """The merges file is neither set nor on the `clip` package path."""


def set_bpe_path(path):
    """Use the merges file at `path` (a gzip text file: one header line, then one `a b` merge per line)."""
    global _bpe_path
    if path is not None and not os.path.isfile(path):
        raise FileNotFoundError(path)
    _bpe_path = path


def bpe_path():
    if _bpe_path is not None:
        return _bpe_path
    from . import __path__ as dirs
    for d in dirs:
        p = os.path.join(d, BPE_NAME)
        if os.path.isfile(p):
            return p
    raise BPENotFound(
        f"clip.tokenize needs the CLIP BPE merges file {BPE_NAME}: call clip.set_bpe_path(<path to it>) or "
        "weclip_vit_comer_amd.install_dropin(reference_root=<reference checkout>) (its clip/ directory holds the file)")


def byte_symbols():
    """[symbol of byte b for b in the vocabulary's order]: printable bytes keep their own code point and come first
    (in byte order); the other 68 bytes follow, mapped in byte order to 256, 257, ..."""
    printable = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    rest = [b for b in range(256) if b not in set(printable)]
    sym = {b: chr(b) for b in printable}
    sym.update({b: chr(256 + i) for i, b in enumerate(rest)})
    return [(b, sym[b]) for b in printable + rest]


def clean(text):
    try:
        import ftfy
        text = ftfy.fix_text(text)
    except ImportError:
        pass
    text = html.unescape(html.unescape(text)).strip()
    return _SPACES.sub(" ", text).strip().lower()


class Tokenizer:
    def __init__(self, path):
        with gzip.open(path, "rt", encoding="utf-8") as fh:
            lines = fh.read().split("\n")
        merges = [tuple(l.split()) for l in lines[1:1 + N_MERGES]]
        merges = [m for m in merges if len(m) == 2]
        order = byte_symbols()
        self.byte_sym = {b: s for b, s in order}
        units = [s for _, s in order]
        vocab = units + [u + "</w>" for u in units] + ["".join(m) for m in merges] + [SOT, EOT]
        self.encoder = {v: i for i, v in enumerate(vocab)}
        self.decoder = {i: v for v, i in self.encoder.items()}
        self.rank = {m: i for i, m in enumerate(merges)}
        self.words = {SOT: [SOT], EOT: [EOT]}

    def bpe(self, word):
        """symbols of one pre-tokenized word (already in byte symbols)."""
        got = self.words.get(word)
        if got is not None:
            return got
        sym = list(word[:-1]) + [word[-1] + "</w>"]
        while len(sym) > 1:
            best, best_rank = None, None
            for pair in zip(sym, sym[1:]):
                r = self.rank.get(pair)
                if r is not None and (best_rank is None or r < best_rank):
                    best, best_rank = pair, r
            if best is None:
                break
            merged, i = [], 0
            while i < len(sym):                      # every occurrence, left to right
                if i + 1 < len(sym) and sym[i] == best[0] and sym[i + 1] == best[1]:
                    merged.append(sym[i] + sym[i + 1])
                    i += 2
                else:
                    merged.append(sym[i])
                    i += 1
            sym = merged
        self.words[word] = sym
        return sym

    def encode(self, text):
        ids = []
        for w in _WORDS.findall(clean(text)):
            w = "".join(self.byte_sym[b] for b in w.encode("utf-8"))
            ids.extend(self.encoder[s] for s in self.bpe(w))
        return ids


def get_tokenizer():
    p = os.path.realpath(bpe_path())
    tok = _cache.get(p)
    if tok is None:
        tok = _cache[p] = Tokenizer(p)
    return tok


def tokenize(texts, context_length=77, truncate=False):
    """(N, context_length) torch.int32: SOT, the BPE ids, EOT, zeros.  A text whose ids do not fit raises
    RuntimeError, or with `truncate` is cut to context_length ids, the last one replaced by EOT."""
    if isinstance(texts, str):
        texts = [texts]
    tok = get_tokenizer()
    sot, eot = tok.encoder[SOT], tok.encoder[EOT]
    out = torch.zeros(len(texts), context_length, dtype=torch.int)
    for i, t in enumerate(texts):
        ids = [sot] + tok.encode(t) + [eot]
        if len(ids) > context_length:
            if not truncate:
                raise RuntimeError(f"Input {t} is too long for context length {context_length}")
            ids = ids[:context_length]
            ids[-1] = eot
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int)
    return out
