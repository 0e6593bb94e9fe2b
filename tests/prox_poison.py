"""One proximity scenario whose outputs must not depend on what device memory held (DESIGN.md sections 50 and 55): run as a script this
file is one child of tests/test_gpu_prox.py::test_outputs_do_not_depend_on_what_memory_held -- `python tests/prox_poison.py OUT_DIR TAG`
in a process whose environment carries AICAM_POISON_ALLOC -- and saves every output array as OUT_DIR/TAG_<key>.npy with the recording
helpers of tests/poison_scenarios.py, the allocation probe's arrays among them.  The pair table is exactly the kind of state that goes
wrong here: resident, read before it is written, and indexed by slots that change hands.  No GPU is touched on import."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import poison_scenarios as P                                            # noqa: E402


def scenario():
    """The planted pair, a three-stream crowd (slots change hands, a reset, a stream that stops) and the ground case, call by call with
    export and export_pairs after every call."""
    import prox_cases as PC
    M = P.pkg("proximity")
    out = {}
    for case in (PC.pair_case(), PC.crowd_case(1, 3, (3, 4, 5)), PC.ground_case(), PC.cliques_case()):
        kw = dict(case["kw"])
        kw["metric"] = "ground" if kw["metric"] == 0 else "body"
        stage = M.Proximity(case["streams"], case["hw"], **kw)
        for i, op in enumerate(case["ops"]):
            tag = f"{case['name']}_op{i}"
            if op[0] == "update":
                P.rec(out, tag, stage.update(op[1], cap=case["cap"], cap_pairs=case["cap_pairs"]))
            elif op[0] == "drain":
                P.rec(out, tag, stage.drain(cap=case["cap"]))
            elif op[0] == "flush":
                P.rec(out, tag, stage.flush(op[1], cap=case["cap"]))
            elif op[0] == "reset":
                stage.reset(op[1])
            elif op[0] == "option":
                stage.option(op[1], op[2])
            elif op[0] == "ground":
                stage.set_ground(op[2], op[3], stream=op[1])
            for s in range(stage.streams):
                P.rec(out, f"{tag}_export{s}", stage.export(s))
                P.rec(out, f"{tag}_pairs{s}", stage.export_pairs(s))
        stage.close()
    return out


def main(argv):
    out_dir, tag = argv[1], argv[2]
    out = {"probe_" + k: v for k, v in P.pkg("_lib").debug_alloc_probe().items()}          # first: nothing this process freed is behind it
    out.update(scenario())
    for k, v in out.items():
        np.save(os.path.join(out_dir, f"{tag}_{k}.npy"), np.asarray(v))


if __name__ == "__main__":
    main(sys.argv)
    sys.exit(0)
