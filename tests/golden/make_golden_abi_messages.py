"""Golden fixture of the trainer's C boundary: what every check before the first launch in csrc/gmz_train.hip,
gmz_heads.hip and gmz_conv.hip returns and reports (tests/test_abi_messages.py holds the case table and the rules).

Run on a machine WITHOUT a GPU, from a build of the commit whose messages are to be the record:
    make -C datou-gomoku-muzero_amd/csrc && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_abi_messages.py
(GMZ_LIB=<path> records another build's libgmz.so.)

Writes tests/golden/abi_messages.json: {case id: [return code, gmz_last_error() text]}.  The committed file was recorded
from the build before the host code of the three files was folded into one check-and-dispatch path per family; it is
the judge of that change and of later ones, so regenerate it only when a message is changed on purpose.

Refuses to record a case that did not fail, or whose text has the shape of a failed HIP call (the stringified call, a
colon, HIP's text, " @<file>:<line>"): that case got through its checks and reached a launch.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))  # tests/ (conftest adds the repository root)

import torch  # noqa: E402

import test_abi_messages as T  # noqa: E402
import datou_gomoku_muzero_amd._lib as L  # noqa: E402


def main():
    if torch.cuda.is_available():
        sys.exit("a GPU is present: the cases use fake pointers and are recorded on a machine without one")
    got = T.run_cases(L.load())
    for cid, (rc, text) in got.items():
        if rc != -1 or not text or T.got_past_validation(text):
            sys.exit("not recorded: case %s returned %d with %r (it must stop at a check)" % (cid, rc, text))
    with open(T.FIXTURE, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases from %s" % (T.FIXTURE, len(got), L.LIB_PATH))


if __name__ == "__main__":
    main()
