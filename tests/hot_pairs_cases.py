"""Corpora for the tests of the hot words' pair-chunks (z_pairs_kernel; tests/test_hot_pair_lists_cpu.py and
tests/test_hot_pairs_gpu.py): the edge rows of the pair-chunk builder in one small corpus."""
import numpy as np

from ldagroupedgibbssampler_amd.corpus import Corpus

HOT = 72          # words 0 .. HOT - 1 are the corpus' most frequent (a hot table of HOT rows holds exactly them), word HOT - 1 the rarest of them: the last row
V = 400


def edges_corpus(seed=7, fillers=240):
    """Documents, in order (the words of a document are shuffled: the builder sorts them by table row):
    one hot word 300 times (a pair of more tokens than a round and than a chunk's cap of 256) | empty | 64 distinct hot words
    once each | empty | 65 distinct | two documents of one hot token among cold ones | 40 and 24 distinct words | 41 and 24 |
    32 words x 4 (128 tokens) | 32 words x 4 and the rarest hot word once (129) | 63 words once, one of them twice, and the
    rarest once (64 pairs, 65 tokens) | then `fillers` documents of 30 random hot tokens and a cold one, every seventh followed by an
    empty document.  Every cold word occurs once, the rarest hot word a few times, every other hot word more often."""
    rng = np.random.default_rng(seed)
    cold = iter(range(HOT, V))
    last = HOT - 1
    docs = [
        [0] * 300,
        [],
        list(range(64)),
        [],
        list(range(65)),
        [5] + [next(cold) for _ in range(20)],
        [next(cold) for _ in range(10)] + [47] + [next(cold) for _ in range(10)],
        list(range(10, 50)), list(range(30, 54)),
        list(range(0, 41)), list(range(47, 71)),
        [w for w in range(32) for _ in range(4)],
        [w for w in range(39, 71) for _ in range(4)] + [last],
        list(range(8, 71)) + [60, last],
    ]
    for j in range(fillers):
        if j % 7 == 3:
            docs.append([])
        docs.append(list(rng.integers(0, HOT - 1, 30)) + [next(cold)])
    toks, ptr = [], [0]
    for d in docs:
        d = np.array(d, np.int32)
        rng.shuffle(d)
        toks.append(d)
        ptr.append(ptr[-1] + len(d))
    c = Corpus(np.array(ptr, np.int64), np.concatenate(toks).astype(np.int32), V)
    freq = np.bincount(c.tokens, minlength=V)
    assert freq[HOT:].max() == 1 < freq[last] < freq[:last].min(), "words 0 .. HOT - 1 are the most frequent, HOT - 1 the rarest of them"
    return c
