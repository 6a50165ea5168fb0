"""Topic priors ("anchor words") of scheme=spalias_priors: the priors file of the cfg key ``topic_prior_filename``.

A restatement of SpaliasUncollapsedParallelWithPriors.extractPriorSpec / calculatePriors / ensureConsistentPriors
(SpaliasUncollapsedParallelWithPriors.java:74-168) as they are written, quirks included:

  * a line is ``topic,word,word,...``; a line whose TRIMMED form is empty or starts with ``#`` is skipped;
  * the line is split on ``,`` and spec[0] goes through Integer.parseInt untouched -- no trimming, so ``" 3"`` is an error;
  * every word of a line joins the keep set of the line's topic and the zero set of every other topic below K; after all
    lines each topic's keep set is taken out of its zero set.  The sets hold the words UNTRIMMED (Java's TreeSets of the
    split's pieces): ``a,x`` and ``b, x`` name two different set members, "x" and " x", that trim to the same word;
  * a word is trimmed only when it is looked up in the vocabulary; a word that is not there is skipped, one warning per word;
  * a line whose topic is >= K keeps nowhere and zeroes its words in every topic.

The result is the sorted list of zero cells (topic, word id): what ggs_set_topic_priors takes.
"""
import re
import sys

import numpy as np

# Integer.parseInt: an optional sign, then decimal digits only (Character.digit accepts any Unicode decimal digit, as \d does)
_JAVA_INT = re.compile(r"[+-]?\d+\Z")
# String.trim(): strips code points <= U+0020 from both ends
_JAVA_TRIM = "".join(chr(i) for i in range(0x21))


def java_trim(s):
    return s.strip(_JAVA_TRIM)


def java_parse_int(s):
    """Integer.parseInt(s): ValueError where Java throws NumberFormatException."""
    if not _JAVA_INT.match(s):
        raise ValueError("Cant extract topic number from: %s" % s)
    v = int(s)
    if not -2 ** 31 <= v < 2 ** 31:
        raise ValueError("Cant extract topic number from: %s" % s)
    return v


def java_split_commas(s):
    """String.split(","): trailing empty strings are removed (a line of commas only gives no piece at all)."""
    parts = s.split(",")
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def extract_prior_spec(lines, num_topics):
    """extractPriorSpec (:124-168): per topic the sorted list of (untrimmed) words to zero out."""
    to_zero = [set() for _ in range(num_topics)]
    to_keep = [set() for _ in range(num_topics)]
    for line in lines:
        t = java_trim(line)
        if t.startswith("#") or len(t) == 0:
            continue
        spec = java_split_commas(line)
        if not spec:                                # "," alone: Java indexes spec[0] of an empty array
            raise ValueError("Cant extract topic number from: %r" % line)
        current = java_parse_int(spec[0])
        for word in spec[1:]:
            for topic in range(num_topics):
                (to_keep if topic == current else to_zero)[topic].add(word)
    return [sorted(to_zero[k] - to_keep[k]) for k in range(num_topics)]


def read_lines(path):
    """Files.readAllLines: lines ended by \\n, \\r\\n or \\r, no empty line behind a final terminator."""
    with open(path, encoding="utf-8", newline="") as f:
        text = f.read()
    lines = re.split(r"\r\n|\n|\r", text)
    if lines and lines[-1] == "":
        lines.pop()
    return lines


def zero_cells(lines, num_topics, vocab, warn=None):
    """calculatePriors (:74-100) + ensureConsistentPriors (:102-121): the sorted zero cells as two int32 arrays
    (topics, words).  ValueError for a topic with every word zero and for words that are zero in every topic."""
    index = {w: i for i, w in enumerate(vocab)}
    num_types = len(vocab)
    warned = set()
    cells = set()
    for topic, words in enumerate(extract_prior_spec(lines, num_topics)):
        for raw in words:
            word = java_trim(raw)
            i = index.get(word)
            if i is None:
                if word not in warned:
                    warned.add(word)
                    msg = 'WARNING: UncollapsedParallelLDA.calculatePriors: Word "%s" does not exist in the dictionary!' % word
                    (warn or (lambda m: print(m, file=sys.stderr)))(msg)
                continue
            cells.add((topic, i))
    per_topic = np.zeros(num_topics, np.int64)
    per_word = np.zeros(num_types, np.int64)
    for k, v in cells:
        per_topic[k] += 1
        per_word[v] += 1
    if num_types and (per_topic == num_types).any():
        raise ValueError("Inconsistent prior spec, one topic has all Zero priors!")
    bad = [vocab[i] for i in np.nonzero(per_word == num_topics)[0]] if num_topics else []
    if bad:
        raise ValueError("Inconsistent prior spec, '[%s]' has all Zero priors!" % ", ".join(bad))
    cells = sorted(cells)
    return (np.asarray([c[0] for c in cells], np.int32), np.asarray([c[1] for c in cells], np.int32))


def load_zero_cells(path, num_topics, vocab, warn=None):
    return zero_cells(read_lines(path), num_topics, vocab, warn)


def priors_matrix(num_topics, num_types, topics, words):
    """getTopicPriors: [K][V], 1.0 everywhere but 0.0 in the zero cells."""
    p = np.ones((num_topics, num_types), np.float64)
    p[np.asarray(topics, np.int64), np.asarray(words, np.int64)] = 0.0
    return p
