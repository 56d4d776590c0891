#!/usr/bin/env python3
"""Records tests/golden/plan_uses.json: what every kind of MFCC plan answers to every use of a plan (tests/plan_uses.py), on a GPU,
at the commit BEFORE the plan's kernel forms and acceptance rules moved into one table -- the behaviour that change has to keep.

    python tests/golden/make_golden_plan_uses.py [out.json]

The matrix is run twice.  A hash is kept only where both runs agree; the cells whose hash was dropped are listed under
"unstable_hashes".  A cell the library answered with DSP_EHIP "invalid configuration" -- a launcher's own fall-through for a kernel
form that does not exist, reached because no host check refused the call -- is marked "now_einval": the closed list of cells whose
answer the change corrects to DSP_EINVAL (a marked stream push: the session is refused at its creation instead)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import plan_uses as P  # noqa: E402


def record(torch, stop_params):
    return {name: P.run_plan(torch, name, stop_params) for name in P.PLAN_NAMES}


def main():
    import torch
    assert torch.cuda.is_available(), "the recorder needs a GPU"
    import dsp_amd
    stop_params = dict(np.load(os.path.join(P.GOLDEN, "stop_model.npz"), allow_pickle=False))
    first, second = record(torch, stop_params), record(torch, stop_params)
    unstable, marked = [], []
    for name in P.PLAN_NAMES:
        for use in P.USES:
            a, b = first[name][use], second[name][use]
            assert (a["rc"], a["error"]) == (b["rc"], b["error"]), (name, use, a, b)
            if a.get("sha256") != b.get("sha256"):
                a["sha256"] = None
                unstable.append(f"{name}/{use}")
            if a["rc"] == P.DSP_EHIP and "invalid configuration" in a["error"]:
                a["now_einval"] = True
                marked.append(f"{name}/{use}")
    out = sys.argv[1] if len(sys.argv) > 1 else P.FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"library": dsp_amd.load().dsp_version().decode(), "unstable_hashes": unstable, "now_einval": marked, "plans": first}, f, indent=1)
        f.write("\n")
    print(f"{out}: {len(P.PLAN_NAMES)} plans x {len(P.USES)} uses; {len(marked)} cells marked now_einval, {len(unstable)} unstable hashes")
    for m in marked:
        print("  now_einval", m, "|", first[m.split('/')[0]][m.split('/')[1]]["error"])


if __name__ == "__main__":
    main()
