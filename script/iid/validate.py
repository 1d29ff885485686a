#!/usr/bin/env python
"""One-pass validation of an IID dataset: predict, score every image on the GPU and write the metric files of eval.py,
see marigold_amd/evaluation/harness.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from marigold_amd.evaluation.harness import validate_iid_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(validate_iid_main())
