"""The maze3d launch-route map (tests/maze_routes.py, a restatement of mg_maze3d_step's choice) against the case lists of
tests/test_maze3d_routes_gpu.py: together they must reach every route of the default library and every knob route. CPU only."""
import maze_routes as mr


def _table(rows):
    return "\n".join("  REC %d  %-7s  %-5s  %d wave%s : %s" % (k[0], k[1], "uint8" if k[2] else "int32", k[3],
                                                               "s" if k[3] > 1 else " ", v) for k, v in rows)


def test_maze3d_route_map_covers_every_route():
    every = mr.default_routes()
    assert len(every) == 24
    hit = {}
    for c in mr.DEFAULT_CASES:
        r = mr.case_route(c)
        hit.setdefault(mr.route_key(r), []).append(c["name"])
    existing = {}
    for n, res, cells, dtype in mr.EXISTING_MAZE_GPU_PARAMS:
        r = mr.maze3d_route(n, res, cells, obs_dtype=dtype)
        existing.setdefault(mr.route_key(r), []).append("%dx%d n=%d%s" % (res[0], res[1], n, "*" if dtype == "uint8" else ""))
    rows = [(k, "new: %s | test_maze_gpu.py: %s" % (",".join(hit.get(k, ["-"])), ",".join(existing.get(k, ["-"]))))
            for k in sorted(every)]
    print("maze3d default-library routes (new oracle cases | existing test_maze_gpu.py parameters):\n" + _table(rows))
    missing = every - set(hit)
    assert not missing, "routes no default case reaches: %s" % sorted(missing)
    assert set(hit) <= every
    print("existing test_maze_gpu.py parameters reach %d of %d routes (* uint8: compared with the GPU's own int32 frame, not the "
          "oracle)" % (len(set(existing) & every), len(every)))

    # every knob route of the knob list is reached by its child's cases
    by_id = {tid: (knob, val, cases) for tid, knob, val, cases in mr.KNOB_CASES}
    lines = []
    for tid, what, pred in mr.required_knob_routes():
        knob, val, cases = by_id[tid]
        names = [c["name"] for c in cases if pred(mr.case_route(c, {knob: val}), c)]
        lines.append("  %s=%s  %-48s : %s" % (knob, val, what, ",".join(names) or "-"))
        assert names, "%s=%s: no case reaches '%s'" % (knob, val, what)
    print("maze3d knob routes:\n" + "\n".join(lines))


def test_maze3d_route_map_restates_the_host_rule():
    """Spot checks of the map itself against the rule in mg_maze3d_step (frame-size thresholds, knob parsing, the stock flags)."""
    r = mr.maze3d_route
    assert r(9, (64, 64), [2.0])["waves"] == 1 and r(9, (64, 65), [2.0])["waves"] == 2
    assert r(9, (127, 129), [2.0])["waves"] == 2 and r(9, (128, 128), [2.0])["waves"] == 4
    assert r(15, (32, 32), [2.0])["rec"] == 1 and r(17, (32, 32), [2.0])["rec"] == 2
    assert r(9, (32, 32), [2.0])["stock"] and r(9, (32, 32), [1.0])["stock"]
    assert not r(9, (32, 32), [0.5])["stock"]                 # text / cell = 2: cells narrower than a texture
    assert not r(9, (32, 32), [1.5])["stock"] and not r(9, (32, 32), [2.0, 1.0])["stock"]
    assert not r(9, (32, 32), [2.0], tex_size=48)["stock"]
    assert not r(9, (32, 32), [2.0], knobs={"MG_MAZE3D_GENERIC": "1"})["stock"]
    assert r(9, (32, 32), [2.0], knobs={"MG_MAZE3D_NO_SMALL": "1"})["small"] is False
    assert r(9, (256, 256), [2.0], knobs={"MG_MAZE3D_WAVES": "1"})["small"] is True
    assert r(9, (32, 32), [2.0], knobs={"MG_MAZE3D_WAVES": "3"})["waves"] == 1        # ignored: not 1, 2 or 4
    assert r(9, (256, 256), [2.0], knobs={"MG_MAZE3D_WAVES": "2,48"})["slab"] == 32   # ignored slab
    assert r(9, (256, 256), [2.0], knobs={"MG_MAZE3D_WAVES": "2,64"})["slab"] == 64
    assert r(9, (32, 32), [2.0], obs_dtype="uint8")["u8"] == "bytes"
    assert r(9, (32, 32), [2.0], obs_dtype="uint8", knobs={"MG_MAZE3D_U8_PACKED": "1"})["u8"] == "packed"
    assert r(9, (32, 30), [2.0], obs_dtype="uint8", knobs={"MG_MAZE3D_U8_PACKED": "1"})["u8"] == "bytes"
    assert r(9, (3, 64), [2.0], knobs={"MG_MAZE3D_WAVES": "4"})["idle_wave_groups"] == 1
