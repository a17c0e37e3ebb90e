"""Child process of tests/test_gpu_streams.py: one group of the scenarios of tests/stream_tools.py (or the two-thread run) in a
fresh process whose environment gives the side stream a hardware queue of its own (GPU_MAX_HW_QUEUES = stream_tools.HW_QUEUES, set
by the parent), results to a JSON file.

    python tests/stream_worker.py GROUP OUT.json          (GROUP: one of stream_tools.groups(), or "threads")
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(group, out):
    import stream_tools as ST
    print(f"stream-worker: group {group}, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}")
    res = ST.run_threads() if group == "threads" else ST.run_group(group)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
