#!/usr/bin/env python3
import os, runpy; runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "fuzz", "fuzz_small_layer.py"), run_name="__main__")
