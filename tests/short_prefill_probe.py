"""Run by tests/test_prefill_fullsize_gpu.py in a fresh process (LLMIE_NO_FUSED_SHORT_PREFILL is read once per process): the
module's CONFIG1 prefills of its seeded 7B-geometry layer in format argv[2]; writes the outputs to argv[1] (.npz)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]
from conftest import load_llmie  # noqa: E402
import test_prefill_fullsize_gpu as m  # noqa: E402

out_path, fmt = sys.argv[1], sys.argv[2]
np.savez(out_path, **m.config1_run(load_llmie(), m.seven_b_weights(), fmt))
