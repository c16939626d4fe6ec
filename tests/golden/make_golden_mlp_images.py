#!/usr/bin/env python3
"""Write tests/golden/mlp_images.npz: every MLP image and streamed pack of the seven configurations, as uint32 words.

    python tests/golden/make_golden_mlp_images.py

The golden records what the image builders of csrc/ngf_mlp_image.hpp produce for the synthetic weights of tests/mlp_image_host.py, through the same
stand-alone program the test runs (tests/host/mlp_image_main.cpp).  It was written at the commit that MOVED the builders out of ngf_field.hip and
ngf_infoinv.hpp unchanged, and the commit that rewrote them from shared pieces had to reproduce it bit for bit; to check that again, run this
script at the tree of the moving commit and compare.  Regenerate it only together with a deliberate change of a layout (ngf_mlp_layout.hpp)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mlp_image_host as H  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as work:
        exe, flags = H.compile_program(work)
        words, sections, _ = H.run_program(exe, work)
    for key, a in words.items():
        print(f"{key}: {a.size} words, {int((a == 0).sum())} zero")
    np.savez_compressed(H.GOLDEN, **words)
    print(f"{H.GOLDEN}: {os.path.getsize(H.GOLDEN)} bytes (program built with {' '.join(flags)})")


if __name__ == "__main__":
    main()
