#!/usr/bin/env python3
"""Records what tests/test_cpp_adapter.py::test_overlay_matches_the_reference_it_replaces checks the drop-in overlay
(include/reference_overlay/) against, so that the test runs without the reference checkout.

    python tests/golden/make_overlay_facts.py <reference checkout>   ->  tests/golden/overlay_facts.json

Facts only, no source text:
  CMakeLists.txt                 its line count and the SHA-256 of every line (what CMakeLists.diff's hunks must match to
                                 apply), and the numbers of the lines that name the source file the diff drops
  the two replaced headers       the targets of their #include lines, whether each carries the namespace / using line the
                                 replacement must keep, and the names of the classes they define
  src/base/jy_ProjectedStateSpace.cpp   the classes whose members it defines
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = (("closed_chain_motion_planner/base/constraints/ConstraintFunction.h", "using namespace std;"),
           ("closed_chain_motion_planner/base/jy_ProjectedStateSpace.h", "namespace ob = ompl::base;"))
DROPPED = "src/base/jy_ProjectedStateSpace.cpp"
INCLUDE = re.compile(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', re.M)
CLASS = re.compile(r"^\s*class\s+(\w+)\s*:", re.M)
MEMBER = re.compile(r"^\w[\w:<> \*&]*?\b(\w+)::\w+\(", re.M)


def line_sha(line):
    return hashlib.sha256(line.encode()).hexdigest()


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_overlay_facts.py <reference checkout>")
    ref = sys.argv[1]
    lines = open(os.path.join(ref, "CMakeLists.txt")).read().split("\n")
    facts = {
        "cmakelists": {"lines": len(lines), "line_sha256": [line_sha(ln) for ln in lines],
                       "lines_naming_dropped_source": [i + 1 for i, ln in enumerate(lines) if DROPPED in ln]},
        "headers": {},
        "dropped_source": {"path": DROPPED,
                           "member_classes": sorted(set(MEMBER.findall(open(os.path.join(ref, DROPPED)).read())))},
    }
    for hdr, keep in HEADERS:
        text = open(os.path.join(ref, "include", hdr)).read()
        facts["headers"][hdr] = {"includes": sorted(set(INCLUDE.findall(text))), "keep": keep, "has_keep": keep in text,
                                 "classes": sorted(set(CLASS.findall(text)))}
    with open(os.path.join(HERE, "overlay_facts.json"), "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
