"""tests/give_up_calls.py against the prototypes of include/lbm_hip.h, without a device: the ledger names every function
whose first parameter is an lbm_ctx* or an lbm_batch* exactly once, names nothing else, and allows exactly the six calls the
header's rule (at lbm_sync) allows on a failed owner.  A new entry point fails here until it has an entry."""
import os
import re

import give_up_calls as ledger
from conftest import ROOT

# a prototype's name and the type of its first parameter: `<name>(lbm_ctx* ...`, `<name>(const lbm_batch* ...`
PROTOTYPE = re.compile(r"\b(lbm_\w+)\s*\(\s*(?:const\s+)?(lbm_ctx|lbm_batch)\s*\*")


def header_entry_points():
    """{"lbm_ctx": [names], "lbm_batch": [names]} in the header's order, comments stripped"""
    with open(os.path.join(ROOT, "include", "lbm_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = {"lbm_ctx": [], "lbm_batch": []}
    for name, owner in PROTOTYPE.findall(text):
        found[owner].append(name)
    return found


def test_the_parser_sees_the_header():
    found = header_entry_points()
    # the first and the last prototype of each owner, and a const first parameter
    assert found["lbm_ctx"][0] == "lbm_rccl_info" and found["lbm_ctx"][-1] == "lbm_tracers_now"
    assert found["lbm_batch"][0] == "lbm_batch_member" and found["lbm_batch"][-1] == "lbm_batch_tracers_now"
    assert "lbm_get_info" in found["lbm_ctx"] and "lbm_batch_get_info" in found["lbm_batch"]
    assert not any(name.startswith("lbm_double_") for names in found.values() for name in names)
    assert not any(name.startswith("lbm_create") for names in found.values() for name in names)


def test_the_ledger_names_every_entry_point_once():
    found = header_entry_points()
    for owner, calls in (("lbm_ctx", ledger.CTX_CALLS), ("lbm_batch", ledger.BATCH_CALLS)):
        names = found[owner]
        assert len(names) == len(set(names)), [n for n in names if names.count(n) > 1]
        assert sorted(set(names) - set(calls)) == [], "entry points of the header without a verdict after a give-up"
        assert sorted(set(calls) - set(names)) == [], "entries that name no function of the header"
    assert not set(ledger.CTX_CALLS) & set(ledger.BATCH_CALLS)      # (two dicts: a name once in each at the most)


def test_exactly_the_six_are_allowed():
    everything = dict(ledger.CTX_CALLS, **ledger.BATCH_CALLS)
    assert all(entry[0] in (ledger.REFUSED, ledger.ALLOWED) and callable(entry[1]) for entry in everything.values())
    allowed = {name for name, entry in everything.items() if entry[0] == ledger.ALLOWED}
    assert allowed == ledger.ALLOWED_CALLS and len(allowed) == 6
    assert allowed == {"lbm_destroy", "lbm_destroy_batch", "lbm_get_info", "lbm_batch_get_info", "lbm_batch_member", "lbm_rccl_info"}
    # a ring reader is a reader with the common signature, and every one of the header is marked
    for calls, prefix in ((ledger.CTX_CALLS, "lbm_read_"), (ledger.BATCH_CALLS, "lbm_batch_read_")):
        rings = ledger.ring_readers(calls)
        assert all(name.startswith(prefix) and calls[name][0] == ledger.REFUSED for name in rings)
    with open(os.path.join(ROOT, "include", "lbm_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    with_n_read = set(re.findall(r"\b(lbm_\w+)\s*\([^;]*\bint\s*\*\s*n_read\s*\)\s*;", text))
    assert with_n_read == set(ledger.ring_readers(ledger.CTX_CALLS) + ledger.ring_readers(ledger.BATCH_CALLS))
    print()
    for owner, calls in (("lbm_ctx*", ledger.CTX_CALLS), ("lbm_batch*", ledger.BATCH_CALLS)):
        for name, entry in calls.items():
            print("%-10s %-30s %s%s" % (owner, name, entry[0], "  (ring reader: *n_read = 0)" if len(entry) > 2 else ""))
    print("later refusal: " + ledger.refusal("<function>"))


def test_the_refusal_names_the_function_and_says_what_is_lost():
    words = ledger.refusal("lbm_read_cells")
    assert words.startswith("lbm_read_cells: ")
    assert "an earlier launch of the resident kernel gave up" in words and "the lattice and the records" in words and "invalid" in words
    # the source holds the words once, as one format
    with open(os.path.join(ROOT, "lbm-asynchronous_amd", "csrc", "lbm_hip.hip")) as f:
        source = f.read()
    literal = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', source[source.index("const char kFailedOwner[]"):].split(";")[0]))
    assert literal == ledger.LATER_REFUSAL.replace("{name}", "%s")
    assert source.count("kFailedOwner") == 2                  # its definition and REFUSE_FAILED
