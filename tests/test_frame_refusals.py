"""The format stage of the trajectory file driver, all of it: for every value of frames_f32 and header_bytes 0 and 8 the
driver answers what tests/golden/frame_refusals.json recorded before the frame source (gpu_frames.hip) took the stage over -
which refusal speaks when several bits are set, and its exact words.  (The per-format suites check one conflicting bit at a
time.)  No GPU and no file: the frame file does not exist."""
import importlib.util
import json
import os

import freesasa_amd as fa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# past the format stage the answer is the machine's: without a device the device list is refused, with one the file is
PAST_THE_FORMAT = ("no HIP device available: libfreesasa_amd has no CPU path", "cannot open the frame file")


def test_every_frames_f32_word_is_refused_as_recorded():
    spec = importlib.util.spec_from_file_location("make_frame_refusals_golden", os.path.join(GOLDEN, "make_frame_refusals_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(os.path.join(GOLDEN, "frame_refusals.json")) as f:
        want = json.load(f)
    assert len(want) == 512 and len({r["message"] for r in want}) >= 20
    got = maker.table(fa.lib())
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["frames_f32"], g["header_bytes"]) == (w["frames_f32"], w["header_bytes"])
        if w["message"] in PAST_THE_FORMAT:
            assert g["rc"] == -1 and g["message"] in PAST_THE_FORMAT, (g, w)
        else:
            assert g == w
