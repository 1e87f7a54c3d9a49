"""The profile log's cost model of the linear family, as a fixture  --  TEST INFRASTRUCTURE.

    ARDAE_LIB=<libardae_hip.so of the commit to record> python tools/gen_linear_profile_costs.py [--out FILE]

Runs on the GPU, under the default knob environment, with the library ARDAE_LIB names (ardae_amd/_lib.py) - a build of the commit
BEFORE a change of the launch layer, so that the fixture pins what that commit reported and not what the changed code reports - and
writes tests/golden/linear_profile_costs.json:

  "recorded_from"   what the library was built from (--commit: a word for the file, the tool cannot know it)
  "cases"           tag of every case of tests/linear_cases.py::TABLE -> sorted [name, calls, flops, bytes] of the profile log after the
                    case's launch through its entry point.  One launch per tag: a case's kernel is asserted by its path and its cost
                    depends on sizes and operands, which the tag spells out, not on the layout or the data (every case of the table is
                    compared with its tag's entry, so a tag whose layouts disagreed would fail there)
  "scenes"          the same for tests/linear_cases.py::SCENES (launchers ardae_linear does not reach)

Flops and bytes are integer-valued doubles far below 2^53; the file holds them as integers.  Names, counts and settings only.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linear_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=C.COSTS_PATH)
    ap.add_argument("--commit", default="the parent commit", help="what ARDAE_LIB was built from, for the file's header")
    a = ap.parse_args()
    assert os.environ.get("ARDAE_LIB"), "name the library to record from in ARDAE_LIB: the fixture must not come from the code under test"
    assert C.knob_env() == ("1", "1", "1", "1"), "record under the default knob environment"
    cases = {}
    for c, kind in C.TABLE:
        if c.tag in cases:
            continue
        inp = C.make_inputs(C.make_data(c, kind), "cuda")
        entries = C._library(inp, per_layer=False)
        head, tail = C.kernel_of(c)
        assert len(entries) == 1 and entries[0]["name"].startswith(head) and entries[0]["name"].endswith(tail), (c.tag, entries)
        cases[c.tag] = C.costs(entries)
    scenes = {name: run() for name, run in sorted(C.SCENES.items())}
    doc = dict(recorded_from=f"{a.commit}: recorded with a separate build of that commit's library (ARDAE_LIB), not with the code these numbers test",
               knob_environment="default", columns=["name", "calls", "flops", "bytes"], cases=cases, scenes=scenes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:       # one case per line
        head = ",\n".join(f" {json.dumps(k)}: {json.dumps(doc[k])}" for k in ("recorded_from", "knob_environment", "columns"))
        body = ",\n".join(f" {json.dumps(sec)}: {{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(doc[sec].items())) + "\n }"
                          for sec in ("cases", "scenes"))
        f.write("{\n" + head + ",\n" + body + "\n}\n")
    assert json.load(open(a.out)) == doc
    print(f"{a.out}: {len(cases)} cases, {sum(len(v) for v in scenes.values())} scene entries, {os.path.getsize(a.out)} bytes")
    for name, v in scenes.items():
        print(name, v)


if __name__ == "__main__":
    main()
