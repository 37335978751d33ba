"""The generated vocabulary the dictionary timing tools share (tools/expand_time.py, tools/suggest_time.py)."""
import numpy as np


def make_vocabulary(n, seed=17):
    """n distinct lowercase words, rank order: frequent words are short (2 .. 4 letters up to rank ~1000), rare
    ones longer (up to 12), letters drawn with English-like weights"""
    rng = np.random.default_rng(seed)
    letters = np.array(list("etaoinshrdlcumwfgypbvkjxqz"))
    p = np.array([12.7, 9.1, 8.2, 7.5, 7.0, 6.7, 6.3, 6.1, 6.0, 4.3, 4.0, 2.8, 2.8, 2.4, 2.4, 2.2, 2.0, 2.0, 1.9, 1.5, 1.0,
                  0.8, 0.15, 0.15, 0.1, 0.07])
    p /= p.sum()
    m = 2 * n
    mat, extra = rng.choice(26, size=(m, 12), p=p), rng.integers(0, 4, size=m)
    words, seen = [], set()
    for i in range(m):
        if len(words) == n:
            break
        length = int(min(12, max(2, np.log2(len(words) + 4) * 0.55 + extra[i])))
        w = "".join(letters[mat[i, :length]])
        if w not in seen:
            seen.add(w)
            words.append(w)
    assert len(words) == n
    return words
