"""The chunk loop that swz_dataset_query and swz_dataset_summarize share, when a reader thread fails in the middle of the stream:
a node file of a chunk behind the first is cut short after the data set was written.  The scan reads headers only, so the call
plans its chunks, streams the first ones and meets the short file in a reader thread.  That is so for BIN and BINZ; the scan of
a LAS data set compares every header's record count with the file's size and refuses the short file by name before a chunk is
read, which is the same to the caller and is held here too.  Which of the two refused is told by the words of the refusal
(WHERE), and by the table that the chunks in front of the short file leave in the workspace of a summarize.

What must hold: the call raises and names the file; swz_dataset_summarize leaves no node-summaries.swz; the context is as
usable as before -- the next query of the intact data set counts what the host counts (bin_read_node and a numpy mask), and
the workspace holds afterwards what the same query leaves on a context that never saw a failure: the call's part of it ("in_*",
"out_*") went back although the call ended in the middle, and no reader thread was left behind to write into it.  A failed
summarize keeps the table of its reduction (as a successful one does), which a query does not touch: there the equality holds
on top of what the context held right after the failure."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
BOX = ([0.125, 0.0625, 0.1875], [0.875, 0.8125, 0.9375])
COLUMNS = ("intensity", "classification")
FORMATS = ("BIN", "BINZ", "LAS")
EXT = {"BIN": ".bin", "BINZ": ".binz", "LAS": ".las"}
# what refuses the short file: the reader threads of the stream (BIN: pread of a piece, BINZ: the file's inflate), or the scan
WHERE = {"BIN": "cannot read the arrays of", "BINZ": "its zlib stream does not hold what its header says",
         "LAS": "the point records pass the end of the file"}
MID_STREAM = ("BIN", "BINZ")
CHUNK = 600
SIDECAR = "node-summaries.swz"


def _cloud():
    """4000 points, none within 2^-10 of a face of BOX: a LAS file's grid (finer than 2^-20 of the node) moves no point across it"""
    rng = np.random.default_rng(1618)
    xyz = rng.random((4400, 3))
    faces = np.concatenate([np.asarray(BOX[0]), np.asarray(BOX[1])])
    near = (np.abs(np.concatenate([xyz, xyz], axis=1) - faces) < 2.0 ** -10).any(axis=1)
    xyz = xyz[~near][:4000]
    assert len(xyz) == 4000
    cols = {"intensity": rng.integers(0, 65535, 4000, endpoint=True).astype(np.uint16),
            "classification": rng.integers(0, 31, 4000, endpoint=True).astype(np.uint8)}
    return xyz, cols


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    import schwarzwald_amd as swz
    root = tmp_path_factory.mktemp("stream_failure")
    dirs = {fmt: str(root / fmt) for fmt in FORMATS}
    with swz.Context(0) as ctx:
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=300, spacing_at_root=swz.spacing_from_diagonal(*UNIT, 12))
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            t.add_batch(*_cloud())
            t.finalize()
            for fmt in FORMATS:
                t.write_output(dirs[fmt], fmt, attrs=COLUMNS)
                t.write_properties(dirs[fmt])
    # the host's count, once: every BIN node file, the closed box
    scan = swz.dataset_scan(dirs["BIN"])["nodes"]
    want = 0
    for level, key in zip(scan["level"], scan["key"]):
        xyz = swz.bin_read_node(os.path.join(dirs["BIN"], swz.node_name(int(level), int(key)) + ".bin"))[0]
        want += int(((xyz >= np.asarray(BOX[0])) & (xyz <= np.asarray(BOX[1]))).all(axis=1).sum())
    assert 1000 < want < 4000
    return dict(dirs=dirs, want=want)


def _cut_a_node_file(swz, directory, fmt):
    """the largest node file of the query's last chunk, cut short behind its header; returns its name.  The table the query
    reads is a part of the one swz_dataset_summarize reads, in the same order: the file is behind the first chunk of both."""
    kept = swz.dataset_query_nodes(directory, *BOX)
    first = swz.output_chunks(kept["count"], CHUNK)
    assert len(first) - 1 >= 3, "three chunks or more"
    k0 = int(first[-2])
    k = k0 + int(np.argmax(kept["count"][k0:]))
    assert kept["count"][k] > 0
    name = swz.node_name(int(kept["level"][k]), int(kept["key"][k])) + EXT[fmt]
    path = os.path.join(directory, name)
    blob = open(path, "rb").read()
    with open(path, "wb") as f:   # BIN, BINZ: the header and two thirds of the arrays or of the zlib stream; LAS: the header and a few records
        f.write(blob[:len(blob) - len(blob) // 3] if fmt != "LAS" else blob[:227 + 40])
    return name


@pytest.mark.parametrize("call", ["query", "summarize"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_short_file_in_a_later_chunk(S, tmp_path, fmt, call):
    import schwarzwald_amd as swz
    good = S["dirs"][fmt]
    bad = str(tmp_path / "bad")
    shutil.copytree(good, bad)
    name = _cut_a_node_file(swz, bad, fmt)
    with swz.Context(0) as ctx, swz.Context(0) as fresh:
        with pytest.raises(swz.SwzError) as e:
            if call == "query":
                swz.dataset_query(ctx, bad, *BOX, chunk_points=CHUNK, return_nodes=True)
            else:
                swz.dataset_summarize(ctx, bad, chunk_points=CHUNK)
        print("%s %s: %s" % (fmt, call, e.value))
        assert name in str(e.value), str(e.value)
        assert ("swz_dataset_" + call) in str(e.value) and WHERE[fmt] in str(e.value)
        assert not os.path.exists(os.path.join(bad, SIDECAR)) and not os.path.exists(os.path.join(bad, SIDECAR + ".tmp"))
        held = ctx.workspace_bytes() if call == "summarize" else 0   # the table of the reduction; a query's arrays are the next query's
        if call == "summarize":   # chunks were reduced before the short file came, or none was streamed at all
            assert (held > 0) == (fmt in MID_STREAM)
        # the same context goes on
        got = swz.dataset_query(ctx, good, *BOX, chunk_points=CHUNK, return_nodes=True)
        assert got["count"] == S["want"] and got["stats"]["chunks"] >= 3
        again = swz.dataset_query(fresh, good, *BOX, chunk_points=CHUNK, return_nodes=True)
        assert again["count"] == S["want"]
        print("workspace: %d after the failure and the query (%d of them the summaries'), %d on a fresh context"
              % (ctx.workspace_bytes(), held, fresh.workspace_bytes()))
        assert fresh.workspace_bytes() > 0
        assert ctx.workspace_bytes() == held + fresh.workspace_bytes()
