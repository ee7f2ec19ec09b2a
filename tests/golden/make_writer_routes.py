#!/usr/bin/env python3
"""Record tests/golden/writer_routes.json: what every route through the stream writer (tests/writer_routes.py) wrote and moved at the commit
the record was taken from -- the yardstick of refactors of fuif_amd/csrc/writer.cpp.  Run it ON THAT COMMIT, never on the code under test,
with the wavefront emulator's library (tests/test_emulated_kernels.py build_emulated_library) so that it needs no GPU:

    FUIF_AMD_LIB=tests/_emu/libfuifgpu_emu.so WRITER_ROUTES_COMMIT=<commit> python tests/golden/make_writer_routes.py

Per case: SHA-256 and length of every picture's stream (and of the streams with the index trailer), and per route that can move planes
the tuples of encode_plane_traffic() and encode_learn_traffic().  All routes of a case must write ONE set of streams; the script stops
where they do not."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fuif_amd  # noqa: E402
import writer_routes  # noqa: E402


def main():
    if "_emu" not in os.path.basename(os.environ.get("FUIF_AMD_LIB", "")):
        raise SystemExit("set FUIF_AMD_LIB to the emulated library of the commit to record")
    fuif_amd.DEFAULT_SPLIT_BITS = writer_routes.SPLIT_BITS     # as tests/conftest.py
    record = {"generator": "tests/golden/make_writer_routes.py", "recorded_at_commit": os.environ.get("WRITER_ROUTES_COMMIT", ""), "cases": {}}
    cases = writer_routes.cases()
    for name in writer_routes.CASE_NAMES:
        entry = {"streams": [], "index_streams": [], "traffic": {}}
        for route, streams, device in writer_routes.routes(fuif_amd, cases[name]):
            have = entry["index_streams" if route.endswith("_index") else "streams"]
            got = [writer_routes.digest(b) for b in streams]
            common = min(len(have), len(got))
            assert have[:common] == got[:common], "%s: route %s writes other bytes than the routes before it" % (name, route)
            have.extend(got[common:])
            if device:
                entry["traffic"][route] = {"plane": list(fuif_amd.encode_plane_traffic()), "learn": list(fuif_amd.encode_learn_traffic())}
        record["cases"][name] = entry
        print("%-24s %d streams, %d routes with traffic" % (name, len(entry["streams"]), len(entry["traffic"])))
    assert record["cases"]["learned_tm1"]["streams"] != record["cases"]["fixed_tm0"]["streams"], "no tree was learned"
    with open(os.path.join(HERE, "writer_routes.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
