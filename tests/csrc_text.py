"""The text of a csrc translation unit together with the shared cutter headers it includes: the statements of the resize, of the
conversion and of the row collection live in those headers, so what a test requires of "the file" it requires of this union."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lightweight-face-detection-centernet_amd", "csrc")
SHARED = ("cf_cutpx.h", "cf_collect.h")


def unit(name):
    """{file: text} of csrc/<name> and of every shared header it includes, directly or through another of them"""
    texts, todo = {}, [name]
    while todo:
        f = todo.pop()
        texts[f] = open(os.path.join(CSRC, f)).read()
        todo += [h for h in SHARED if '#include "%s"' % h in texts[f] and h not in texts and h not in todo]
    return texts


def assert_one_statement(texts, needs):
    """every call of `needs` appears somewhere in the union; no file of it restates the resize or the conversion or calls an atomic"""
    union = "\n".join(texts.values())
    for call in needs:
        assert call in union, call
    for f, text in texts.items():
        assert "1220542" not in text and not re.search(r"\brintf\b", text), f      # no second statement of either
        assert not re.search(r"\batomic\w*\s*\(", text, flags=re.I) and "__hip_atomic" not in text, f      # prefix sums, no atomic call
