"""examples/evaluate_opt_dataset.cpp over the device context, in the Region + Depth configuration or, with --texture,
with the texture modality the reference's example runs: 552 single-body sequences, tracked from the first image's ground truth, ADD against the body's diameter:

    python tools/evaluate_opt_dataset.py [--batch N] [--judge-on-device] [--texture] [--texture-match auto|one|tiled]
                                         OPT_DIR EXTERNAL_DIR [body ...]

OPT_DIR holds Model3D/<body>/<body>.obj and 3D/<sequence>/{color,depth}/NNNN.png, 3D/poses/<sequence>.txt;
EXTERNAL_DIR receives models/.  The diameters are computed on the device over all vertices of every mesh
(m3t_hip_vertices_diameter), not taken from a table.  --batch N: up to N bodies share one context, each with its own
cameras and its own list of sequences (default: all six).  --judge-on-device: ADD is formed on the device
(m3t_hip_judge_set_add_only), no wait and no pose read per frame.  --texture: every body also carries the texture
modality of the reference's example (set_use_texture_modality(true)) with the library's built-in detector in ORB's place
(evaluation.evaluate_opt_dataset, use_texture_modality): the reference's configuration with another detector, not its
numbers.  --texture-match: the form of the Hamming match (the library's developer override M3T_HIP_TEXTURE_MATCH); every form gives the same results.
Prints the area under curve per sequence, per body and overall."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("3dobjecttracking_amd")


def report(title, result):
    print("%s: area_under_curve = %g" % (title, result["area_under_curve"]))


# one process per GPU (torch.distributed.run or any launcher that sets these): every process takes its share of runs
rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
local_rank = int(os.environ.get("LOCAL_RANK", "0"))

if __name__ == "__main__":
    argv = sys.argv[1:]
    judge_on_device = "--judge-on-device" in argv
    if judge_on_device:
        argv.remove("--judge-on-device")
    batch = len(pkg.evaluation.OPT_BODY_NAMES)
    if "--batch" in argv:
        at = argv.index("--batch")
        batch = int(argv[at + 1])
        del argv[at:at + 2]
    kw = {}
    if "--texture" in argv:
        argv.remove("--texture")
        kw["use_texture_modality"] = True
    if "--texture-match" in argv:
        at = argv.index("--texture-match")
        if at + 1 >= len(argv) or argv[at + 1] not in ("auto", "one", "tiled"):
            sys.exit("--texture-match takes auto, one or tiled")
        os.environ["M3T_HIP_TEXTURE_MATCH"] = argv[at + 1]  # (a context looks at it when it is made)
        del argv[at:at + 2]
    if len(argv) < 2:
        sys.exit("usage: evaluate_opt_dataset.py [--batch N] [--judge-on-device] [--texture] "
                 "[--texture-match auto|one|tiled] OPT_DIR EXTERNAL_DIR [body ...]")
    body_names = argv[2:] or list(pkg.evaluation.OPT_BODY_NAMES)
    _, final = pkg.evaluation.evaluate_opt_dataset(lambda: pkg.open_context(local_rank), argv[0], argv[1], body_names,
                                                   report=report, shard=(rank, world), batch=batch,
                                                   judge_on_device=judge_on_device, **kw)
    for name in body_names + ["all"]:
        if name in final:
            report(name, final[name])
