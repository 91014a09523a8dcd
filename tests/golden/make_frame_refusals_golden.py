"""Records frame_refusals.json: what freesasa_gpu_trajectory_file answers for every value of frames_f32 (0 .. 255) and
header_bytes 0 and 8, with a frame file that does not exist, five atoms and one device - the return code and the whole
message.  Which refusal speaks when several bits of frames_f32 are set is part of the interface; the table was recorded with
the library as it was BEFORE the frame source (gpu_frames.hip) took over the format stage, and tests/test_frame_refusals.py
replays it.  Run from the repository root with a built library:  python tests/golden/make_frame_refusals_golden.py"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import freesasa_amd as fa  # noqa: E402

FRAMES = b"/nonexistent/freesasa_amd/frames"
N_ATOMS = 5


def refusal(L, bits, header_bytes):
    radii = np.full(N_ATOMS, 1.5)
    err = C.create_string_buffer(512)
    rc = L.freesasa_gpu_trajectory_file(FRAMES, bits, header_bytes, radii.ctypes.data_as(C.POINTER(C.c_double)), N_ATOMS, 0, fa.LEE_RICHARDS, 1.4, 20, 0,
                                        b"/nonexistent/freesasa_amd/totals", b"/nonexistent/freesasa_amd/sasa", None, 0, 0, None, err, 512)
    return int(rc), err.value.decode()


def table(L):
    return [dict(zip(("frames_f32", "header_bytes", "rc", "message"), (bits, hb) + refusal(L, bits, hb))) for hb in (0, 8) for bits in range(256)]


if __name__ == "__main__":
    rows = table(fa.lib())
    with open(os.path.join(ROOT, "tests", "golden", "frame_refusals.json"), "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print(len(rows), "entries,", len({r["message"] for r in rows}), "distinct messages")
