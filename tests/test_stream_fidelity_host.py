"""The table of tests/test_gpu_stream_fidelity.py against include/marigold_hip.h, on the CPU: every function whose prototype ends in
``void* stream)`` is a row of the table or one of its documented exclusions, so that an entry point added later cannot be forgotten.
The header is parsed as text, not compiled."""
import os
import re

from tests import test_gpu_stream_fidelity as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "marigold_hip.h")) as f:
        return f.read()


def _prototypes_with_a_trailing_stream(text):
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    return re.findall(r"\b(mg_\w+)\s*\(([^;{}()]*\bvoid\s*\*\s*stream\s*)\)\s*;", code)


def test_the_parser_finds_what_it_should():
    text = "/* int mg_commented(void* stream); */\nint mg_a(const float* x,\n   void* stream);\nint mg_b(void* stream, float s);\nint mg_c(int n);"
    assert [name for name, _ in _prototypes_with_a_trailing_stream(text)] == ["mg_a"]


def test_every_prototype_with_a_stream_is_a_row_or_a_documented_exclusion():
    names = [name for name, _ in _prototypes_with_a_trailing_stream(_header())]
    assert len(names) == len(set(names)) and len(names) >= 40
    known = set(T.ROWS) | set(T.OUT_OF_SCOPE)
    assert not [n for n in names if n not in known], "a call with a stream that tests/test_gpu_stream_fidelity.py does not know"
    assert not (set(T.ROWS) | set(T.OUT_OF_SCOPE)) - set(names), "the table names a function the header does not declare with a trailing stream"
    assert not set(T.ROWS) & set(T.OUT_OF_SCOPE)
    # every synchronising call is a row that skips parts 2 to 4, or excluded as a model program; mg_model_predict_next takes its
    # stream before the strength and is no prototype of the list above
    assert all(n in known or n == "mg_model_predict_next" for n in T.SYNCHRONISES)
    assert [n for n in T.ROWS if n in T.SYNCHRONISES] == ["mg_ensemble_depth"] and "mg_ensemble_depth" not in T.ASYNC_ROWS
    assert set(T.NEIGHBOUR) == set(T.ROWS) and all(T.NEIGHBOUR[n] != n and T.NEIGHBOUR[n] in T.ASYNC_ROWS for n in T.ROWS)


def test_the_sentences_about_synchronising_are_the_headers():
    flat = re.sub(r"\s*\n\s*\*\s*", " ", _header())   # (comment lines joined: a sentence may wrap)
    for name, sentence in T.SYNCHRONISES.items():
        assert sentence in flat, (name, sentence)


def test_the_header_names_the_test():
    assert "tests/test_gpu_stream_fidelity.py" in _header()
