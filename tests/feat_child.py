"""Child process of test_gpu_feat.py::test_bit_reproducible_across_contexts_and_processes: the same sequences in a fresh process, their digest on stdout."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import __graft_entry__ as graft  # noqa: E402

graft.load_package()

if __name__ == "__main__":
    from test_gpu_feat import run_chain
    from mvil_fusion_amd import lib
    print("digest " + run_chain(lib.load_vilsolve()))
