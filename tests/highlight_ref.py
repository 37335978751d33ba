"""highlight_fragments and make_snippet of the reference (index/highlight.rs:11-80) restated line for line over
bytes with Python's `re`: re.A | re.I stands for the regex crate's case-insensitive matching on ASCII input (for
ASCII texts and words of [0-9A-Za-z_] the two agree: \\b, \\W and the case folding only ever look at ASCII),
pattern.search(text, pos) for find_at (the look-behind of \\b sees the byte in front of pos), leftmost-first
alternation is what both engines do.  NOT the token-run shortcut the device builds: the tests compare the two."""
import re


def highlight_fragments(text: bytes, terms, phrases, pre_tag: bytes, post_tag: bytes, fragment_size: int,
                        number_of_fragments: int):
    if len(text) == 0 or (len(terms) == 0 and len(phrases) == 0):      # :17-19
        return []
    patterns = []
    for phrase in phrases:                                              # :22-32 phrase patterns first
        if len(phrase) == 0:
            continue
        patterns.append(rb"\b" + rb"\W+".join(re.escape(bytes(p)) for p in phrase) + rb"\b")
    for term in terms:                                                  # :33-38
        if len(term) == 0:
            continue
        patterns.append(rb"\b" + re.escape(bytes(term)) + rb"\b")
    if not patterns:                                                    # :39-41
        return []
    rx = re.compile(b"|".join(patterns), re.A | re.I)                   # :42-45
    out = []
    offset = 0
    for _ in range(number_of_fragments):                                # :48
        m = rx.search(text, offset)                                     # :49 find_at
        if m is None:
            break
        start = m.start() - min(m.start(), fragment_size // 2)          # :50 saturating_sub
        end = min(len(text), start + fragment_size)                     # :51
        fragment = text[start:end]                                      # :52 a string of its own
        out.append(rx.sub(lambda c: pre_tag + c.group(0) + post_tag, fragment))  # :53-57 replace_all
        offset = m.end()                                                # :59
    return out


def make_snippet(text: bytes, terms, phrases):                          # :67-80
    frags = highlight_fragments(text, terms, phrases, b"**", b"**", 120, 1)
    return frags.pop() if frags else None


def highlight_spec_ref(text: bytes, spec: dict):
    """The fragments of one text under a searchlite_amd.highlight spec dict."""
    return highlight_fragments(text, spec["terms"], spec["phrases"], spec["pre_tag"], spec["post_tag"],
                               spec["fragment_size"], spec["number_of_fragments"])
