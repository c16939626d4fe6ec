"""The marching-cubes case table of csrc/ngf_mesh.hip, derived rather than typed in.

Corner ``c = x + 2y + 4z``; bit c of a case is set when corner c is INSIDE (value >= level).  The 12 edges are the corner pairs that
differ in one bit, numbered ``4 * axis + r`` with the edge's lower corner ("base", the lattice point that owns it) taken in rising order:
x edges from corners 0 2 4 6, y edges from 0 1 4 5, z edges from 0 1 2 3.

Per case and per cube face the crossing edges are joined by segments: two crossing edges are joined; four (an ambiguous face) are joined
so that each inside corner of the face is cut off on its own -- a rule that reads the face's four signs only, so the two cells that share
the face draw the same segments.  Every segment is directed with the inside corners on its left, seen from outside the cube, so the
segments close into directed loops.  A loop is triangulated as a fan whose start is chosen so that no diagonal joins two edges of one cube
face (such a diagonal lies IN the face, where the neighbouring cell may draw it again: a mesh edge used by four triangles).  Triangles
wind so that their normals point to the outside (low) side.

This is the usual vertex definition (one vertex per sign-changing lattice edge) but NOT the triangulation of skimage's Lewiner tables.

``python -m ngf_amd.mesh_table`` prints the header csrc/ngf_mesh_table.hpp; tests/test_mesh_cpu.py compares the two."""
from __future__ import annotations

MAX_TRIS = 5

EDGE_AXIS = [a for a in range(3) for _ in range(4)]
EDGE_BASE = [b for a in range(3) for b in range(8) if not b >> a & 1]
EDGE_CORNERS = [(b, b | 1 << a) for a, b in zip(EDGE_AXIS, EDGE_BASE)]
_EDGE_OF = {frozenset(p): e for e, p in enumerate(EDGE_CORNERS)}


def _face_cycle(axis, side):
    """The four corners of a face, counter-clockwise seen from outside the cube."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    cyc = [(side << axis) | (du << u) | (dv << v) for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1))]
    return cyc if side else cyc[::-1]


FACES = [_face_cycle(a, s) for a in range(3) for s in range(2)]
# the cube faces an edge lies in, as a bit mask over FACES
EDGE_FACES = [sum(1 << f for f, cyc in enumerate(FACES) if c0 in cyc and c1 in cyc) for c0, c1 in EDGE_CORNERS]


def face_segments(case, cyc):
    """Directed segments (edge_from, edge_to) of one face: one per maximal run of inside corners, from the edge behind the run to the edge
    in front of it (the run is then on the segment's left, seen from outside)."""
    ins = [case >> c & 1 for c in cyc]
    if sum(ins) in (0, 4):
        return []
    segs = []
    for m in range(4):
        if ins[m] and not ins[m - 1]:                      # a run starts at m
            n = m
            while ins[(n + 1) % 4]:
                n += 1
            e_to = _EDGE_OF[frozenset((cyc[m - 1], cyc[m]))]
            e_from = _EDGE_OF[frozenset((cyc[n % 4], cyc[(n + 1) % 4]))]
            segs.append((e_from, e_to))
    return segs


def case_loops(case):
    """The directed loops of a case, each as a list of edges starting at its smallest edge; loops in rising order of that edge."""
    nxt = {}
    for cyc in FACES:
        for a, b in face_segments(case, cyc):
            assert a not in nxt, "an edge leaves twice"
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), "segments do not close"
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def in_face(e0, e1):
    return bool(EDGE_FACES[e0] & EDGE_FACES[e1])


def fan(loop):
    """Triangles of a loop as a fan; the first start (in loop order) none of whose diagonals lies in a cube face."""
    n = len(loop)
    for s in range(n):
        r = loop[s:] + loop[:s]
        if not any(in_face(r[0], r[i]) for i in range(2, n - 1)):
            return [(r[0], r[i], r[i + 1]) for i in range(1, n - 1)]
    raise AssertionError(f"no fan without an in-face diagonal for loop {loop}")


def _outward(case_tris):
    """True when the triangles of the one-corner case wind with normals pointing away from corner 0."""
    mid = [[(((c0 >> a & 1) + (c1 >> a & 1)) / 2) for a in range(3)] for c0, c1 in EDGE_CORNERS]
    p, q, r = (mid[e] for e in case_tris[0])
    u, v = [q[a] - p[a] for a in range(3)], [r[a] - p[a] for a in range(3)]
    n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    return sum(n) > 0


def build():
    """(loops[256], tris[256]): per case the list of directed loops and the list of triangles (edge triples)."""
    loops = [case_loops(c) for c in range(256)]
    reverse = not _outward(fan(loops[1][0]))
    tris = []
    for c in range(256):
        t = [tri for loop in loops[c] for tri in fan(loop)]
        tris.append([tri[::-1] for tri in t] if reverse else t)
        assert len(tris[-1]) <= MAX_TRIS
    return loops, tris


LOOPS, TRIS = build()
TRI_COUNT = [len(t) for t in TRIS]


def header_text():
    rows = []
    for c in range(256):
        flat = [e for tri in TRIS[c] for e in tri]
        flat += [-1] * (3 * MAX_TRIS - len(flat))
        rows.append("    {" + ", ".join(f"{e:2d}" for e in flat) + "},")
    counts = [", ".join(str(n) for n in TRI_COUNT[r:r + 32]) for r in range(0, 256, 32)]
    return ("// ngf_mesh_table.hpp -- GENERATED by ngf_amd/mesh_table.py (python -m ngf_amd.mesh_table); tests/test_mesh_cpu.py regenerates and compares it.\n"
            "// Marching-cubes cases: bit c of a case = corner c (x + 2y + 4z) is inside; edge 4 * axis + r, owned by corner {0 2 4 6 | 0 1 4 5 | 0 1 2 3}[r].\n"
            "#pragma once\n"
            "namespace ngf {\n"
            f"static constexpr int kMeshMaxTris = {MAX_TRIS};\n"
            "static __device__ const unsigned char kMeshTriCount[256] = {\n" + "".join(f"    {r},\n" for r in counts) + "};\n"
            f"static __device__ const signed char kMeshTris[256][{3 * MAX_TRIS}] = {{\n" + "\n".join(rows) + "\n};\n"
            "}  // namespace ngf\n")


if __name__ == "__main__":
    print(header_text(), end="")
