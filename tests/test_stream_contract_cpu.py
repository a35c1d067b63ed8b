"""The stream-contract table (tests/stream_contract.py) against the headers and against the GPU module's case registries.  No GPU."""
import re

import pytest

from mcm_amd import abi
from tests import stream_contract as sc


def test_every_entry_with_a_stream_has_a_class_and_nothing_else_has():
    entries = sc.stream_entries()
    product = {**abi.PROTOTYPES, **abi.EXTENSION_PROTOTYPES}
    assert entries and entries <= set(product), sorted(entries - set(product))   # read the same declarations the binding reads
    assert not entries & (set(abi.HARNESS_PROTOTYPES) | set(abi.EXTENSION_HARNESS_PROTOTYPES))
    # a `stream` is the last parameter and a pointer; an entry whose last parameter is no pointer cannot be one that was missed
    import ctypes
    assert all(product[n][1][-1] is ctypes.c_void_p for n in entries)
    missing, stale = sorted(entries - set(sc.CONTRACT)), sorted(set(sc.CONTRACT) - entries)
    assert not missing, f"entries that take a stream and have no row in tests/stream_contract.py: {missing}"
    assert not stale, f"rows of tests/stream_contract.py that are no exported entry with a stream: {stale}"


def test_every_row_has_a_class_and_a_reason_that_cites_a_line():
    for name, row in sc.CONTRACT.items():
        cls, why = row
        assert cls in sc.CLASSES, name
        assert re.search(r":\d+", why), f"{name}: the reason cites no line"
    assert {n for c in sc.CLASSES for n in sc.classes(c)} == set(sc.CONTRACT)


def test_the_parser_reads_declarations_as_the_binding_does():
    text = """/* int mcm_in_comment(void* stream); */
    int mcm_a(mcm_handle* h, void* stream);
    int mcm_b(mcm_handle* h, int32_t streams);
    #ifdef MCM_HARNESS
    int mcm_debug_c(mcm_handle* h, void* stream);
    #endif
    int mcm_d(const mcm_handle* h,
              const float* x /* [B] */, void* stream);
    """
    import os
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        for name in sc.HEADERS:
            with open(os.path.join(d, name), "w") as f:
                f.write(text if name == "mcm.h" else "int mcm_e(void* stream);\n")
        assert sc.stream_entries(d) == {"mcm_a", "mcm_d", "mcm_e"}


def test_the_gpu_module_has_a_replay_case_for_the_replayable_rows_only():
    pytest.importorskip("torch")
    from tests import test_gpu_stream_contract as g   # importing it touches no GPU

    assert sorted(g.REPLAY_CASES) == sc.classes(sc.REPLAYABLE)
    # ... and an eager-ordering case for every entry that cannot be captured but is asynchronous
    assert set(sc.classes(sc.HOST_STAGED)) <= set(g.ORDER_CASES) <= set(sc.classes(sc.HOST_STAGED) + sc.classes(sc.REPLAYABLE))
    # the entries with a pixel_format run in both
    for entry, (_, variants) in g.REPLAY_CASES.items():
        if entry in ("mcm_encode_image_ex", "mcm_encode_image_x2", "mcm_score_x2", "mcm_encode_image_local"):
            assert set(variants) == {g.F32, g.U8}, entry
        if entry in ("mcm_score_topk", "mcm_score_glmcm"):
            assert {v[0] for v in variants} == {g.F32, g.U8}, entry


def _header_texts():
    import os

    for name in sc.HEADERS:
        with open(os.path.join(os.path.dirname(abi.HEADER_PATH), name)) as f:
            yield name, f.read()


def test_the_header_names_the_class_of_every_entry():
    """Every entry's comment — the last comment block that starts a line before the declaration — closes with "Stream contract:
    <class>", and the "Stream contract" block of include/mcm.h lists the host_staged and the synchronising entries by name."""
    seen = {}
    for header, text in _header_texts():
        code = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m[0]), text, flags=re.S)   # comments blanked, offsets kept
        blocks = list(re.finditer(r"^/\*.*?\*/", text, flags=re.S | re.M))
        for name in sc.CONTRACT:
            decl = re.search(r"\b%s ?\(" % name, code)
            if not decl:
                continue
            before = [b for b in blocks if b.end() <= decl.start()]
            tags = re.findall(r"Stream contract: (\w+)", before[-1][0]) if before else []
            assert tags == [sc.CONTRACT[name][0]], f"include/{header}: the comment above {name} says {tags}"
            seen[name] = tags[0]
    assert set(seen) == set(sc.CONTRACT)
    block = re.search(r"Stream contract —.*?\*/", dict(_header_texts())["mcm.h"], flags=re.S)[0]
    staged = re.search(r"host_staged\b(.*?)\n \*   synchronising\b(.*?)\n \* ONE STREAM", block, flags=re.S)
    assert sorted(re.findall(r"mcm_\w+", staged[1])) == sc.classes(sc.HOST_STAGED)
    assert sorted(re.findall(r"mcm_\w+", staged[2])) == sc.classes(sc.SYNCHRONISING)
