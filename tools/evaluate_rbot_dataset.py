"""examples/evaluate_rbot_dataset.cpp over the device context (region modality; the sequences without modelled
occlusions, with --modeled-occlusions also the reference's fifth column):

    python tools/evaluate_rbot_dataset.py [--batch N] [--judge-on-device] [--modeled-occlusions] [--texture]
                                          RBOT_DATASET_DIR EXTERNAL_DIR [body ...]

--batch N: up to N runs share one device context (each with its own body, model, camera and optimizer); a lost body is
reset alone (m3t_hip_reset_bodies), so the results are those of one context per run.
--judge-on-device: the 5 cm / 5 degree judgement and the reset are the device's (m3t_hip_judge_bodies): no wait and no
pose read per frame; "complete cycle" is then the loop's wall time per frame.
--modeled-occlusions: d_occlusion once more behind the four sequences, with squirrel_small tracked along
poses_second.txt and modelled occlusions on both region modalities (evaluation.evaluate_rbot_dataset,
sequence_occlusions); without the flag the output is that of the four sequences alone.
--texture: every run also carries a texture modality with the built-in detector (use_texture_modality_ of the
reference's evaluator; evaluation.evaluate_rbot_dataset, use_texture_modality); not together with --modeled-occlusions.
Prints the success rate and the mean step time per (sequence, body) and overall, like
RBOTEvaluator::VisualizeFinalResult."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("3dobjecttracking_amd")


def report(title, result):
    print("-" * 80)
    print("%s:\nsuccess rate = %g\ncomplete cycle = %g us" % (title, result["tracking_success"], result["complete_cycle"]))


# one process per GPU (torch.distributed.run or any launcher that sets these): every process takes its share of runs
rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
local_rank = int(os.environ.get("LOCAL_RANK", "0"))

if __name__ == "__main__":
    argv = sys.argv[1:]
    batch = 1
    judge_on_device = "--judge-on-device" in argv
    if judge_on_device:
        argv.remove("--judge-on-device")
    modeled = "--modeled-occlusions" in argv
    if modeled:
        argv.remove("--modeled-occlusions")
    texture = "--texture" in argv
    if texture:
        argv.remove("--texture")
    if texture and modeled:
        sys.exit("--texture cannot be combined with --modeled-occlusions")
    if "--batch" in argv:
        at = argv.index("--batch")
        if at + 1 >= len(argv) or not argv[at + 1].isdigit() or int(argv[at + 1]) < 1:
            sys.exit("--batch takes a positive number of runs per context")
        batch = int(argv[at + 1])
        del argv[at:at + 2]
    if len(argv) < 2:
        sys.exit("usage: evaluate_rbot_dataset.py [--batch N] [--judge-on-device] [--modeled-occlusions] [--texture] "
                 "RBOT_DATASET_DIR EXTERNAL_DIR [body ...]")
    ev = pkg.evaluation
    bodies = argv[2:] or ev.RBOT_BODY_NAMES
    kw = {}
    if modeled:  # evaluate_rbot_dataset.cpp:17-20
        kw = dict(sequence_names=ev.RBOT_SEQUENCE_NAMES + ("d_occlusion",), sequence_occlusions=[False] * 4 + [True])
    if texture:
        kw["use_texture_modality"] = True
    _, overall = ev.evaluate_rbot_dataset(lambda: pkg.open_context(local_rank), argv[0], argv[1], bodies, report=report,
                                          shard=(rank, world), batch=batch, judge_on_device=judge_on_device, **kw)
    report("all_sequences_all_bodies", overall)
