"""CPU suite: the policy of the detectors' device-table cache (blah2_amd/csrc/table_cache.hpp) compiled on its own for the
host with the address and undefined-behaviour sanitizers and driven with a fake device that records its calls
(tests/host/emulate_table_cache.cpp): eight unpinned tables least recently used first, pins that stay, the refusal under
capture before anything is built, one synchronisation in front of an eviction, and failures that leave the list as it was
and nothing allocated.  Every run ends with free_all, so a table left behind is the leak sanitizer's report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = "capturing,alloc24,upload"  # a miss on a stream: the capture test, then the table of three doubles


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("table_cache") / "emulate_table_cache")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-o", path,
                           os.path.join(ROOT, "tests", "host", "emulate_table_cache.cpp")])
    return path


def run(exe, ops):
    """The program on ``ops`` and ``f`` -> one dict per op (the last one is free_all's)."""
    ops = ops.split() + ["f"]
    out = subprocess.run([exe, *ops], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr  # a clean exit: no sanitizer report, no leak
    assert out.stderr == ""
    lines = out.stdout.splitlines()
    assert len(lines) == len(ops)
    rows = []
    for op, line in zip(ops, lines):
        head, err = line.split(" err=", 1)
        f = head.split(" ")
        assert f[0] == op
        row = dict(kv.split("=", 1) for kv in f[1:])
        row.update(op=op, err=err, rc=int(row["rc"]), live=int(row["live"]), built=int(row["built"]),
                   events=[e for e in row["events"].split(",") if e], list=[e for e in row["list"].split(",") if e])
        rows.append(row)
    last = rows[-1]
    assert last["list"] == [] and last["live"] == 0  # free_all leaves nothing
    return rows


def test_a_miss_builds_and_uploads_a_hit_only_hands_out(exe):
    r = run(exe, "g5 g5 g6")
    assert [x["rc"] for x in r[:3]] == [0, 0, 0]
    assert r[0]["events"] == MISS.split(",") and r[0]["out"] == "1005" and r[0]["built"] == 1
    assert r[1]["events"] == [] and r[1]["out"] == "1005" and r[1]["built"] == 1  # a hit touches no device call
    assert r[2]["list"] == ["5", "6"] and r[2]["live"] == 2
    assert r[3]["events"] == ["free", "free"]


def test_ninth_unpinned_insert_evicts_the_oldest_after_one_synchronise(exe):
    r = run(exe, " ".join(f"g{k}" for k in range(1, 10)) + " g1")
    for x in r[:8]:
        assert "sync" not in x["events"] and "free" not in x["events"]
    assert r[7]["list"] == [str(k) for k in range(1, 9)] and r[7]["live"] == 8
    ninth = r[8]
    assert ninth["rc"] == 0 and ninth["out"] == "1009"
    assert ninth["events"].count("sync") == 1 and ninth["events"].count("free") == 1
    assert ninth["events"].index("sync") < ninth["events"].index("free")  # enqueued work may still read the table
    assert ninth["list"] == [str(k) for k in range(2, 10)] and ninth["live"] == 8
    again = r[9]  # key 1 is gone: built anew, and key 2 leaves
    assert again["built"] == 10 and again["list"] == [str(k) for k in range(3, 10)] + ["1"] and again["live"] == 8


def test_pinned_entries_survive_and_do_not_count(exe):
    ops = "p100 p101 p102 " + " ".join(f"g{k}" for k in range(1, 31))
    r = run(exe, ops)
    for x in r[3:11]:  # eight unpinned ones beside the three pins: no eviction yet
        assert "sync" not in x["events"]
    assert r[10]["live"] == 11
    for x in r[11:33]:
        assert x["events"].count("sync") == 1 and x["events"].count("free") == 1 and x["live"] == 11
    last = r[32]["list"]
    assert [e for e in last if e.endswith("p")] == ["100p", "101p", "102p"]
    assert [e for e in last if not e.endswith("p")] == [str(k) for k in range(23, 31)]
    # a ninth PINNED insert evicts nothing either
    r = run(exe, " ".join(f"g{k}" for k in range(1, 9)) + " p9")
    assert "sync" not in r[8]["events"] and r[8]["live"] == 9 and r[8]["list"][-1] == "9p"


def test_a_hit_reorders_and_keeps_its_pin(exe):
    r = run(exe, "g1 p2 g3 g2 g1 p1 g1 " + " ".join(f"g{k}" for k in range(10, 19)))
    assert r[2]["list"] == ["1", "2p", "3"]
    assert r[3]["list"] == ["1", "3", "2p"] and r[3]["events"] == []  # moved to the back, still pinned
    assert r[4]["list"] == ["3", "2p", "1"]
    assert r[5]["list"] == ["3", "2p", "1p"]  # a hit that pins
    assert r[6]["list"] == ["3", "2p", "1p"] and r[6]["built"] == 3  # an unpinned hit does not unpin
    assert r[15]["list"][:2] == ["2p", "1p"] and "3" not in r[15]["list"]  # nine more: 3 was the oldest unpinned one
    assert all(x["built"] == 3 for x in r[3:7])


def test_a_larger_table_serves_a_smaller_request_where_the_caller_says_so(exe):
    r = run(exe, "g16 G12 g12 G20")
    assert r[1]["out"] == "1016" and r[1]["events"] == [] and r[1]["list"] == ["16"]
    assert r[2]["out"] == "1012" and r[2]["list"] == ["16", "12"]  # equality wanted: a table of its own
    assert r[3]["out"] == "1020" and r[3]["built"] == 3


def test_a_miss_while_capturing_is_refused_and_builds_nothing(exe):
    r = run(exe, "g1 c2 c1 p2 c2")
    assert r[1]["rc"] == -1 and r[1]["events"] == ["capturing"] and r[1]["built"] == 1 and r[1]["out"] == "-"
    assert "_prepare" in r[1]["err"] and r[1]["list"] == ["1"] and r[1]["live"] == 1
    assert r[2]["rc"] == 0 and r[2]["events"] == []  # a hit is served under capture, without asking the stream
    assert r[4]["rc"] == 0 and r[4]["out"] == "1002" and r[4]["list"] == ["1", "2p"]  # prepared, then captured


@pytest.mark.parametrize("op,rc,events,err", [("b", -7, ["capturing"], ""), ("a", -2, ["capturing", "alloc24"], "table upload: out of memory"),
                                              ("u", -2, ["capturing", "alloc24", "upload", "free"], "table upload: upload refused")])
def test_a_failure_leaves_the_list_as_it_was_and_leaks_nothing(exe, op, rc, events, err):
    full = " ".join(f"g{k}" for k in range(1, 9))
    for before in ("g1 p2", full):  # also at a full list: nothing is evicted for a table that does not arrive
        n = len(before.split())
        r = run(exe, f"{before} {op}50 g50")
        was = r[n - 1]
        bad = r[n]
        assert bad["rc"] == rc and bad["events"] == events and bad["err"] == err and bad["out"] == "-"
        assert bad["list"] == was["list"] and bad["live"] == was["live"]
        assert r[n + 1]["rc"] == 0 and r[n + 1]["out"] == "1050"  # the same key afterwards: a plain miss


def test_a_failed_synchronise_evicts_and_inserts_nothing(exe):
    r = run(exe, " ".join(f"g{k}" for k in range(1, 9)) + " s9")
    bad = r[8]
    assert bad["rc"] == -2 and bad["events"] == MISS.split(",") + ["sync", "free"] and "device lost" in bad["err"]
    assert bad["list"] == r[7]["list"] and bad["live"] == 8
