"""Which build of the stage kernels a launch takes (difflexmm_amd/csrc/dfx_builds.h: select_fwd_build, select_adj_build, build_code) and the
model x contact dispatcher under it (dfx_dispatch.h: with_physics, with_index), pinned on the CPU: a g++ program around the two headers
prints the selection for a list of queries.  The engine instantiates what these functions select and reports what build_code derives from
them (dfx_stats.tile_kernels), so the GPU tests that assert "this build really ran" stand on this table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r"""
#include <cstdio>
#include "dfx_builds.h"
using namespace dfx;
template <bool (*Served)(int, int)> static void served() {
  for (int m = 0; m < 4; ++m)
    for (int c = 0; c < 3; ++c) {
      int gm = -1, gc = -1;
      const bool ok = with_physics<Served>(m, c, [&](auto M, auto C) { gm = M(); gc = C(); });
      printf("%d", ok && gm == m && gc == c ? 1 : (!ok && gm == -1 ? 0 : 9));
    }
  printf("\n");
}
int main() {
  served<all_physics>();
  served<loop_physics>();
  for (int i = -1; i <= 6; ++i) { int got = -1; const bool ok = with_index<6>(i, [&](auto I) { got = I(); }); printf("%d", ok ? got : 9); }
  printf(" %d\n", (int)with_physics<all_physics>(4, 0, [](auto, auto) {}) + (int)with_physics<all_physics>(0, 3, [](auto, auto) {}));
  int v[18], i, in_buf, out_buf, y_buf, mode, local_only;
  for (;;) {
    for (int k = 0; k < 18; ++k) if (scanf("%d", &v[k]) != 1) return 0;
    if (scanf("%d %d %d %d %d %d", &i, &in_buf, &out_buf, &y_buf, &mode, &local_only) != 6) return 1;
    BuildQuery q;
    q.model = v[0]; q.contact = v[1]; q.n_npb = v[2]; q.n_ovf = v[3]; q.s = v[4]; q.pack3 = v[5]; q.wt = v[6]; q.stage_builds = v[7];
    q.k_uniform = v[8]; q.l_dict_on = v[9]; q.l_dict_lds = v[10]; q.damping_uniform = v[11]; q.t_steps = v[12]; q.AD = v[13]; q.clock = v[14];
    q.records = v[15]; q.fn_tab = v[16]; q.g_b = v[17];
    const FwdBuild f = select_fwd_build(q, i, in_buf, out_buf, y_buf, mode);
    const AdjBuild a = select_adj_build(q, i, local_only);
    printf("%d %d %d %d %d %d %d  %d %d %d %d %d %d  %d %d\n", f.npb, f.tab, f.ovf, f.wt, f.istage, f.recs, (int)f.packed_grid, (int)a.kind, a.npb, a.tab,
           a.wt, a.istage, (int)a.packed_grid, build_code(q, false), build_code(q, true));
  }
}
"""

FIELDS = ["model", "contact", "n_npb", "n_ovf", "s", "pack3", "wt", "stage_builds", "k_uniform", "l_dict_on", "l_dict_lds", "damping_uniform",
          "t_steps", "AD", "clock", "records", "fn_tab", "g_b"]
LINEARIZED, NONLINEAR, SIMPLE_SPRING, STRETCH_TORSION = 0, 1, 2, 3          # dfx_physics.h, BondModel
NONE, ANGLE, DISTANCE = 0, 1, 2                                            # include/dfx.h, DFX_CONTACT_*
GENERIC, BOND_GRADS, REBUILD, OVF = 0, 1, 2, 3                             # dfx_builds.h, AdjKind
LIGAMENT = [(m, c) for m in (NONLINEAR, LINEARIZED) for c in (NONE, ANGLE)]
# the common shape, table on, no clock, six stages, quads, write-through on
BASE = dict(model=NONLINEAR, contact=ANGLE, n_npb=4, n_ovf=0, s=6, pack3=0, wt=1, stage_builds=1, k_uniform=1, l_dict_on=1, l_dict_lds=1,
            damping_uniform=1, t_steps=0, AD=0, clock=0, records=1, fn_tab=1, g_b=0)


def parent_code(q):
    """kernel_build_code as it stood before the selector existed (with its callers' prefix for the reverse sweep): a second statement of the
    rule, which build_code must agree with everywhere but in the one corner it had wrong (3-node blocks on the quad mapping)."""
    model_ok = q["model"] in (NONLINEAR, LINEARIZED) and q["contact"] != DISTANCE
    quad_or_packed = not q["n_ovf"] and (q["n_npb"] == 4 or q["pack3"])
    shape = q["k_uniform"] and q["l_dict_on"] and q["l_dict_lds"] and q["damping_uniform"] and not q["t_steps"] and not q["AD"] and not q["clock"]
    fwd = 2 if (model_ok and quad_or_packed and q["wt"] and q["stage_builds"] and q["fn_tab"] and shape and q["s"] <= 6) else 0
    return fwd, (0 if (q["g_b"] or q["AD"]) else fwd)


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_build_select")
    src, exe = d / "select.cpp", d / "select"
    src.write_text(HARNESS)
    # the plain host compiler: the two headers take no HIP
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "difflexmm_amd", "csrc"), "-o", str(exe), str(src)])

    def run(queries):
        """queries: (fields, i, in_buf, out_buf, y_buf, mode, local_only) -> dicts fwd / adj / code per query"""
        text = "\n".join(" ".join(str(int(q[f])) for f in FIELDS) + " " + " ".join(str(x) for x in rest) for q, *rest in queries)
        lines = subprocess.check_output([str(exe)], input=text + "\n", text=True).splitlines()
        out = []
        for line in lines[3:]:
            x = [int(t) for t in line.split()]
            out.append((dict(npb=x[0], tab=x[1], ovf=x[2], wt=x[3], istage=x[4], recs=x[5], packed=x[6]),
                        dict(kind=x[7], npb=x[8], tab=x[9], wt=x[10], istage=x[11], packed=x[12]), (x[13], x[14])))
        assert len(out) == len(queries)
        return lines[:3], out
    return run


def records_bufs(i):
    return (i, -1 - i, -2 - i, -1, 0, 0)


def stage_bufs(i, s=6):
    return (i, 0 if i == 0 else 1 + ((i - 1) & 1), 0 if i == s - 1 else 1 + (i & 1), 0, 0, 0)


def step(select, q, bufs=records_bufs, stages=None, local_only=0, mode=None):
    """the selections of the stages of one step and the two codes (which do not depend on the stage)"""
    qs = []
    for i in (range(q["s"]) if stages is None else stages):
        b = list(bufs(i))
        if mode is not None:
            b[4] = mode
        b[5] = local_only
        qs.append((q, *b))
    _, out = select(qs)
    codes = {o[2] for o in out}
    assert len(codes) == 1
    return [o[0] for o in out], [o[1] for o in out], codes.pop()


def triple(f):
    return (f["npb"], f["tab"], f["wt"])


def test_dispatcher_serves_what_its_predicate_says(select):
    head, _ = select([])
    assert head[0] == "1" * 12                                  # every model x contact pair, each with its own template arguments
    assert head[1] == "110" "110" "000" "000"                   # linearised and nonlinear ligaments, contact none / angle
    assert head[2] == "90123459 0"                              # stage index 0 .. 5; an unknown model or contact serves nothing


@pytest.mark.parametrize("model,contact", LIGAMENT)
def test_ligament_quads(select, model, contact):
    q = dict(BASE, model=model, contact=contact)
    fwd, adj, code = step(select, q)
    for i in range(6):
        assert triple(fwd[i]) == (4, 1, 1) and fwd[i]["istage"] == i and fwd[i]["recs"] == 1 and not fwd[i]["ovf"] and not fwd[i]["packed"]
        assert adj[i] == dict(kind=GENERIC, npb=4, tab=1, wt=1, istage=i, packed=0)
    assert code == (2, 2) == parent_code(q)
    # stage buffers, and records elsewhere than in this stage's places of the checkpoint (the recompute launches): RECS = 0
    fwd_s, _, _ = step(select, dict(q, records=0), bufs=stage_bufs)
    fwd_r, _, _ = step(select, q, bufs=lambda i: (i, -1 if i == 0 else i, i + 1, -1, 0, 0))
    for f in fwd_s + fwd_r:
        assert triple(f) == (4, 1, 1) and f["istage"] >= 0 and f["recs"] == 0
    # mode 1 (the last stage also writes the checkpoint) keeps the per-stage build, RECS = 0
    fwd_m, _, _ = step(select, q, mode=1)
    assert all(f["istage"] == i and f["recs"] == 0 for i, f in enumerate(fwd_m))

    q0 = dict(q, wt=0)
    fwd, adj, code = step(select, q0)
    assert all(triple(f) == (4, 1, 0) and f["istage"] == -1 for f in fwd)
    assert all(a == dict(kind=GENERIC, npb=4, tab=1, wt=0, istage=-1, packed=0) for a in adj)
    assert code == (0, 0) == parent_code(q0)

    for wt in (0, 1):
        qn = dict(q, fn_tab=0, wt=wt)
        fwd, adj, code = step(select, qn)
        assert all(triple(f) == (4, 0, 0) and f["istage"] == -1 for f in fwd)
        assert all(a == dict(kind=GENERIC, npb=4, tab=0, wt=0, istage=-1, packed=0) for a in adj)
        assert code == (0, 0) == parent_code(qn)
    # an adaptive clock: the table is not read
    fwd, _, code = step(select, dict(q, clock=1))
    assert all(triple(f) == (4, 0, 0) and f["istage"] == -1 for f in fwd) and code[0] == 0

    _, adj, _ = step(select, q, local_only=1)
    assert all(a == dict(kind=GENERIC, npb=4, tab=0, wt=0, istage=-1, packed=0) for a in adj)


@pytest.mark.parametrize("model,contact", [(m, DISTANCE) for m in range(4)] + [(m, c) for m in (SIMPLE_SPRING, STRETCH_TORSION) for c in (NONE, ANGLE)])
def test_other_physics_keeps_the_generic_builds(select, model, contact):
    q = dict(BASE, model=model, contact=contact)
    fwd, adj, code = step(select, q)
    assert all(triple(f) == (4, 1, 1) and f["istage"] == -1 for f in fwd)
    assert all(a == dict(kind=GENERIC, npb=4, tab=1, wt=1, istage=-1, packed=0) for a in adj)
    assert code == (0, 0) == parent_code(q)


@pytest.mark.parametrize("change", [dict(k_uniform=0), dict(l_dict_lds=0), dict(l_dict_on=0, l_dict_lds=0), dict(damping_uniform=0), dict(t_steps=1),
                                    dict(stage_builds=0)], ids=lambda c: "-".join(c))
@pytest.mark.parametrize("n_npb,pack3", [(4, 0), (3, 1), (3, 0)])
def test_outside_the_common_shape(select, change, n_npb, pack3):
    q = dict(BASE, n_npb=n_npb, pack3=pack3, **change)
    fwd, adj, code = step(select, q)
    want = (3, 1, 0) if pack3 else (4, 1, 1)               # (the packed mapping has no generic write-through build)
    assert all(triple(f) == want and f["istage"] == -1 and f["packed"] == pack3 for f in fwd)
    assert all(a == dict(kind=GENERIC, npb=want[0], tab=1, wt=want[2], istage=-1, packed=pack3) for a in adj)
    assert code == (0, 0) == parent_code(q)


@pytest.mark.parametrize("model,contact", LIGAMENT)
def test_three_node_blocks(select, model, contact):
    q = dict(BASE, model=model, contact=contact, n_npb=3, pack3=1)
    fwd, adj, code = step(select, q)
    for i in range(6):
        assert triple(fwd[i]) == (3, 1, 1) and fwd[i]["istage"] == i and fwd[i]["recs"] == 1 and fwd[i]["packed"] == 1
        assert adj[i] == dict(kind=GENERIC, npb=3, tab=1, wt=1, istage=i, packed=1)
    assert code == (2, 2) == parent_code(q)

    q0 = dict(q, wt=0)
    fwd, adj, code = step(select, q0)
    assert all(triple(f) == (3, 1, 0) and f["istage"] == -1 and f["packed"] == 1 for f in fwd)
    assert all(a == dict(kind=GENERIC, npb=3, tab=1, wt=0, istage=-1, packed=1) for a in adj)
    assert code == (0, 0) == parent_code(q0)
    fwd, adj, _ = step(select, dict(q, fn_tab=0))
    assert all(triple(f) == (3, 0, 0) and f["packed"] == 1 for f in fwd) and all((a["npb"], a["tab"], a["wt"], a["packed"]) == (3, 0, 0, 1) for a in adj)

    # the error-estimate launch of the adaptive controller (mode & 2) keeps the quad mapping
    fwd, _, _ = step(select, q, mode=2)
    assert all(triple(f) == (4, 1, 1) and f["istage"] == i and f["recs"] == 0 and f["packed"] == 0 for i, f in enumerate(fwd))

    # DFX_PACK3=0: the quad mapping, and there the per-stage builds run -- the one corner where the code reported before (0) was not what ran
    qq = dict(q, pack3=0)
    fwd, adj, code = step(select, qq)
    for i in range(6):
        assert triple(fwd[i]) == (4, 1, 1) and fwd[i]["istage"] == i and fwd[i]["packed"] == 0
        assert adj[i] == dict(kind=GENERIC, npb=4, tab=1, wt=1, istage=i, packed=0)
    assert code == (2, 2) and parent_code(qq) == (0, 0)
    qq0 = dict(qq, wt=0)
    fwd, _, code = step(select, qq0)
    assert all(triple(f) == (4, 1, 0) and f["istage"] == -1 for f in fwd)
    assert code == (0, 0) == parent_code(qq0)


@pytest.mark.parametrize("model", range(4))
def test_three_node_blocks_with_distance_contact_keep_the_quad_mapping(select, model):
    q = dict(BASE, model=model, contact=DISTANCE, n_npb=3, pack3=1)
    fwd, adj, code = step(select, q)
    assert all(triple(f) == (4, 1, 1) and f["istage"] == -1 and f["packed"] == 0 for f in fwd)
    assert all(a == dict(kind=GENERIC, npb=4, tab=1, wt=1, istage=-1, packed=0) for a in adj)
    assert code == (0, 0) == parent_code(q)


@pytest.mark.parametrize("model", range(4))
@pytest.mark.parametrize("contact", (NONE, ANGLE, DISTANCE))
def test_general_bond_lists(select, model, contact):
    for n_npb, pack3 in ((4, 0), (3, 1)):
        q = dict(BASE, model=model, contact=contact, n_ovf=5, g_b=1, n_npb=n_npb, pack3=pack3)        # (the engine wants g_b with them)
        fwd, adj, code = step(select, q)
        npb = 0 if contact == DISTANCE else 4                   # npb 0: nothing is launched
        assert all(f == dict(npb=npb, tab=0, ovf=1, wt=0, istage=-1, recs=1, packed=0) for f in fwd)
        assert all(a == dict(kind=OVF, npb=npb, tab=0, wt=0, istage=-1, packed=0) for a in adj)
        assert code == (0, 0) == parent_code(q)


@pytest.mark.parametrize("model,contact", LIGAMENT + [(SIMPLE_SPRING, DISTANCE)])
def test_bond_gradients_and_stage_checkpoint(select, model, contact):
    for n_npb, pack3 in ((4, 0), (3, 1)):
        q = dict(BASE, model=model, contact=contact, n_npb=n_npb, pack3=pack3, g_b=1)
        _, adj, code = step(select, q)
        assert all(a == dict(kind=BOND_GRADS, npb=4, tab=0, wt=0, istage=-1, packed=0) for a in adj)
        assert code[1] == 0 and code == parent_code(q)          # (the forward sweep does not read g_b)
        q = dict(BASE, model=model, contact=contact, n_npb=n_npb, pack3=pack3, AD=1, records=0)
        fwd, adj, code = step(select, q, bufs=stage_bufs)
        assert all(a == dict(kind=REBUILD, npb=4, tab=0, wt=0, istage=-1, packed=0) for a in adj)
        assert all(f["istage"] == -1 for f in fwd)
        assert code == (0, 0) == parent_code(q)
        _, adj, _ = step(select, dict(q, g_b=1), bufs=stage_bufs)
        assert all(a["kind"] == BOND_GRADS for a in adj)


@pytest.mark.parametrize("model,contact", LIGAMENT)
def test_a_seventh_stage_has_no_build_of_its_own(select, model, contact):
    q = dict(BASE, model=model, contact=contact, s=7)
    fwd, adj, code = step(select, q)
    assert all(fwd[i]["istage"] == i and adj[i]["istage"] == i for i in range(6))
    assert triple(fwd[6]) == (4, 1, 1) and fwd[6]["istage"] == -1
    assert adj[6] == dict(kind=GENERIC, npb=4, tab=1, wt=1, istage=-1, packed=0)
    assert code == (0, 0) == parent_code(q)
    q4 = dict(q, s=4)
    assert step(select, q4)[2] == (2, 2) == parent_code(q4)


def test_codes_agree_with_the_earlier_rule_over_the_whole_grid(select):
    """every combination of the switches of the rule: build_code against the rule as kernel_build_code stated it, which was right except for
    3-node blocks on the quad mapping with write-through on"""
    import itertools
    qs = []
    for model, contact, (n_npb, pack3), n_ovf, wt, sb, shape, ad, clock, tab, gb, s in itertools.product(
            range(4), range(3), ((4, 0), (3, 1), (3, 0)), (0, 3), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (4, 6, 7)):
        if clock and tab:
            continue                                        # the table is a fixed-grid matter: no adaptive clock beside it (use_fn_table)
        qs.append(dict(BASE, model=model, contact=contact, n_npb=n_npb, pack3=pack3, n_ovf=n_ovf, wt=wt, stage_builds=sb, k_uniform=shape, AD=ad,
                       clock=clock, fn_tab=tab, g_b=gb, s=s))
    _, out = select([(q, 0, 0, 0, 0, 0, 0) for q in qs])
    n_corner = 0
    for q, o in zip(qs, out):
        corner = q["n_npb"] == 3 and not q["pack3"] and not q["n_ovf"]
        if corner and o[2] != parent_code(q):
            n_corner += 1
            qq = dict(q, n_npb=4)
            assert o[2] == parent_code(qq), q                   # what quads report: the same kernels run
        else:
            assert o[2] == parent_code(q), q
    assert n_corner > 0
