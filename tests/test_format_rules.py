"""What a pixel format is to the host code, pinned: the library's host-only format functions -- rsr_image_bytes, rsr_image_span and the five
rsr_out_size* -- answer every case of tests/golden/format_rules.json as the build the file was recorded from did (return value, ow, oh and
the rsr_last_error text of every refusal).  The grid and the recorder are tests/golden/make_format_rules.py; no GPU is touched."""
import hashlib
import importlib.util
import json
import os

import pytest

import realsr_ncnn_vulkan_amd as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_format_rules", os.path.join(GOLDEN, "make_format_rules.py"))
rules = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rules)


@pytest.fixture(scope="module")
def recorded():
    with open(rules.OUT) as f:
        return json.load(f)


def test_the_file_was_recorded_over_this_grid(recorded):
    sha = hashlib.sha256()
    for case in rules.cases():
        sha.update(repr(case).encode())
    assert sha.hexdigest() == recorded["args_sha256"]
    assert set(recorded["answers"]) == {"rsr_image_bytes", "rsr_image_span", "rsr_out_size", "rsr_out_size_yuv", "rsr_out_size_xy", "rsr_out_size_yuv_xy",
                                        "rsr_out_size_fmt"}


def test_the_library_answers_every_recorded_case_identically(recorded):
    L = R.lib()
    wrong = []
    for (name, args), want in zip(rules.cases(), rules.expand(recorded)):
        got = rules.ask(L, name, args)
        got = {"no": list(got)} if isinstance(got, tuple) and isinstance(got[1], str) else (list(got[1:]) if isinstance(got, tuple) else got)
        if got != want:
            wrong.append((name, args, want, got))
    assert not wrong, "%d of the recorded answers changed, the first: %r" % (len(wrong), wrong[:5])


def test_every_valid_format_has_accepted_and_refused_cases(recorded):
    """An over-pruned grid cannot hide a family: per valid format, every entry point that takes a format both accepts and refuses; and the
    entry points without a format argument do both as well."""
    seen = {}
    for (name, args), a in zip(rules.cases(), rules.expand(recorded)):
        key = (name, args[0]) if name in ("rsr_image_bytes", "rsr_image_span", "rsr_out_size_fmt") else (name, None)
        seen.setdefault(key, set()).add(isinstance(a, dict))
    for name in ("rsr_image_bytes", "rsr_image_span", "rsr_out_size_fmt"):
        for fmt in rules.VALID:
            assert seen[(name, fmt)] == {False, True}, (name, fmt)
        for fmt in set(rules.FORMATS) - set(rules.VALID):
            assert seen[(name, fmt)] == {True}, (name, fmt)
    for name in ("rsr_out_size", "rsr_out_size_yuv", "rsr_out_size_xy", "rsr_out_size_yuv_xy"):
        assert seen[(name, None)] == {False, True}, name
    assert os.path.getsize(rules.OUT) < os.path.getsize(os.path.join(GOLDEN, "cases.npz"))
