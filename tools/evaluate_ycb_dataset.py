"""examples/evaluate_ycb_dataset.cpp over the device context (region + depth modality with measured occlusions,
single-region models, tracking from the first keyframe's ground truth):

    python tools/evaluate_ycb_dataset.py [--judge-on-device] [--texture] [--texture-match auto|one|tiled]
                                         YCB_VIDEO_DIR EXTERNAL_DIR [sequence_id ...]

EXTERNAL_DIR holds poses/ground_truth/<sequence>_<body>.txt (the reference ships them as data/ycb-video_poses.zip)
and receives models/.  --judge-on-device: ADD / ADD-S are formed on the device (m3t_hip_judge_bodies), no wait and no
pose read per frame; the execution time is then the loop's wall time per keyframe.
--texture: every run also carries the texture modality of the reference's example (set_use_texture_modality(true)) with
the library's built-in detector in ORB's place (evaluation.evaluate_ycb_dataset, use_texture_modality): the reference's
configuration with another detector, not its numbers.  --texture-match: the form of the Hamming match
(the library's developer override M3T_HIP_TEXTURE_MATCH); every form gives the same results.
Prints ADD / ADD-S AUC and the mean step time per (sequence, body) and overall."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("3dobjecttracking_amd")

BODY_NAMES = ["002_master_chef_can", "003_cracker_box", "004_sugar_box", "005_tomato_soup_can", "006_mustard_bottle",
              "007_tuna_fish_can", "008_pudding_box", "009_gelatin_box", "010_potted_meat_can", "011_banana",
              "019_pitcher_base", "021_bleach_cleanser", "024_bowl", "025_mug", "035_power_drill", "036_wood_block",
              "037_scissors", "040_large_marker", "051_large_clamp", "052_extra_large_clamp", "061_foam_brick"]


def report(title, result):
    print("%s: execution_time = %g us, add auc = %g, adds auc = %g" %
          (title, result["complete_cycle"], result["add_auc"], result["adds_auc"]))


# one process per GPU (torch.distributed.run or any launcher that sets these): every process takes its share of runs
rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
local_rank = int(os.environ.get("LOCAL_RANK", "0"))

if __name__ == "__main__":
    judge_on_device = "--judge-on-device" in sys.argv
    if judge_on_device:
        sys.argv.remove("--judge-on-device")
    kw = {}
    if "--texture" in sys.argv:
        sys.argv.remove("--texture")
        kw["use_texture_modality"] = True
    if "--texture-match" in sys.argv:
        i = sys.argv.index("--texture-match")
        if i + 1 >= len(sys.argv) or sys.argv[i + 1] not in ("auto", "one", "tiled"):
            sys.exit("--texture-match takes auto, one or tiled")
        os.environ["M3T_HIP_TEXTURE_MATCH"] = sys.argv[i + 1]  # (a context looks at it when it is made)
        del sys.argv[i:i + 2]
    if len(sys.argv) < 3:
        sys.exit("usage: evaluate_ycb_dataset.py [--judge-on-device] [--texture] [--texture-match auto|one|tiled] "
                 "YCB_VIDEO_DIR EXTERNAL_DIR [sequence_id ...]")
    sequence_ids = [int(x) for x in sys.argv[3:]] or list(range(48, 60))  # evaluate_ycb_dataset.cpp:13
    _, overall = pkg.evaluation.evaluate_ycb_dataset(lambda: pkg.open_context(local_rank), sys.argv[1], sys.argv[2], sequence_ids,
                                                     BODY_NAMES, report=report, shard=(rank, world),
                                                     judge_on_device=judge_on_device, **kw)
    report("all sequences, all bodies", overall)
