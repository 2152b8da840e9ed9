"""The command line of the analyses, replayed against tests/golden/cli_transcript.json: the hand-written command lines of
tests/golden/make_cli_transcript.py, run with the checker build from the repository root, must give the exit status, the standard output
and the messages that were recorded (and capi.run() the same bytes or the same exception), line for line."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_cli_transcript as mk  # noqa: E402


@pytest.fixture(scope="module")
def ora(built):
    return mk.load_checker()


def test_the_list_covers_what_it_must():
    ls = mk.lines()
    heads = [h.split("=")[0] for h in mk.HEADS]
    assert len(heads) == 13 and len(ls) > 500
    for i, a in enumerate(mk.HEADS):
        assert "--gpus 2 %s @P" % a in ls
        for b in mk.HEADS[i + 1:]:
            assert "%s %s @P" % (a, b) in ls
    for name in ("curves", "dist", "assoc", "trait", "tree", "qtrait", "cluster", "permanova", "mantel", "gainloss", "coevo"):
        assert name in ls and name + " @G" in ls  # no file: the usage; the defaults (or the missing mandatory option)


def test_replay(ora):
    with open(os.path.join(GOLD, "cli_transcript.json")) as f:
        want = json.load(f)
    ls = mk.lines()
    assert [e["line"] for e in want] == ls, "the transcript was recorded from another list: run tests/golden/make_cli_transcript.py on the commit it describes"
    bad = []
    for e in want:
        got = mk.record(e["line"], ora)
        if got != e:
            bad.append("%s\n  recorded: %r\n  now:      %r" % (e["line"], {k: v for k, v in e.items() if got.get(k) != v}, {k: v for k, v in got.items() if e.get(k) != v}))
    assert not bad, "%d of %d lines differ:\n%s" % (len(bad), len(want), "\n".join(bad[:40]))
