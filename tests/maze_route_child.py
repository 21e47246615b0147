"""Child process of tests/test_maze3d_routes_gpu.py: runs maze_routes.run_case on the JSON list of cases in argv[1] under the
MG_MAZE3D_* knob its parent put in the environment (the library reads the knobs once per process), and prints one line
`MAZE_ROUTE_CHILD <json list of per-case summaries>`. A transition mismatch raises (non-zero exit, traceback on stderr)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import maze_routes  # noqa: E402


def main():
    import torch
    assert torch.cuda.is_available(), "the route child needs a GPU"
    cases = json.loads(sys.argv[1])
    out = []
    for c in cases:
        out.append(maze_routes.run_case(c))
    torch.cuda.synchronize()
    print("MAZE_ROUTE_CHILD " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
