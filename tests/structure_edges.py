"""The case tables of the structure code's size and topology edges (csrc/m3t_links.hip: the wave-level LDLT, the MODE 0
link kernels, the five tracking_step_tree_* kernels), the builders of their structures and the helpers that run a case.

No test lives here.  tests/test_structure_edge_cases.py (CPU) runs every case through the oracle alone and checks that it
is *live*, that the tables cover what they claim, and the oracle itself against a float64 restatement;
tests/test_gpu_structure_solves.py runs SOLVE_CASES on the device (link sums injected between
CalculateOptimizationBegin and CalculateOptimizationEnd, no images); tests/test_gpu_structure_edges.py runs TRACK_CASES
through every launch shape of SHAPES with images.  Both compare with the oracle bit for bit.

A structure is a list of `Link` rows (parent index, free directions, body, joint poses) made by the builders `chain`,
`star`, `pad` and `fixed_root`, plus Constraint / SoftConstraint rows.  What the host derives from it is restated here:

  * `tree_work_floats` (m3t_links.hip): the work arrays of a structure; the MODE 0 kernels keep them in LDS while the
    largest structure's fit 152 KB, else in global scratch (UploadTreeTables: ctx->tree_lds);
  * `ldlt_branch` (ldlt_solve_any): n <= 8, <= 13, <= 16 the register variants, above the general routine;
  * `TrackCase.expect`, per launch shape the kernel and [workgroups, parts, threads] the host must report, from
    UploadTreeTables (tree_fused_possible: at most 16 links and size 64 per structure), ComputeLayout (off_hist >= 0: up
    to 16 bins the pair table is staged in LDS), TreeStepLds, TreeStepFused (staged table, >= 63 Newton steps, more
    than 160 KB of LDS: per-sub-step launches, kernel ""), TreeStepSegmented (the same without the Newton-step rule) and
    StepTreeFused (constrained structures keep one workgroup per link; the split kernel needs >= 4 bins and a part's
    elements within its share of 256 lanes; M3T_HIP_TREE_PARTS limits the parts).
"""
import ctypes as C
import types

import numpy as np

import bench_chain
import fused_edges
import scenes
import util
from util import host, syn

FREE, FIXED = (1,) * 6, (0,) * 6
ROT_Z = (0, 0, 1, 0, 0, 0)
# joints of 1, 4, 5 and 6 free directions, rotation and translation mixed, the rendered chains' rotation about z among them
JOINT = {1: ROT_Z, 4: (1, 0, 1, 0, 1, 1), 5: (1, 1, 1, 0, 1, 1), 6: FREE}
TIKHONOV = (1000.0, 30000.0)

LDS_WORK_LIMIT_FLOATS = 152 * 1024 // 4  # UploadTreeTables: tree_work_max * 4 <= 152 KB
FUSED_MAX_LINKS, FUSED_MAX_SIZE = 16, 64  # M3T_TREE_FUSED_MAX_LINKS / _SIZE
LANE_FIELDS = 9                           # M3T_TREE_LANE_FIELDS
LINK_DEV_BYTES = 272                      # sizeof(LinkDev): 59 ints / floats, padded to 8, four pointers
CU_LDS_BYTES = 160 * 1024
COMPUTE_CUS = 256


def tree_work_floats(n_links, dof, n_rows):
    """m3t_links.hip, tree_work_floats"""
    size = dof + n_rows
    return (n_links * (12 * dof + 42 + 72) + size * size + 4 * size + n_rows * (dof + 1) + 2 * 6 * 6 + 64 +
            n_links * (dof * dof + dof) + dof + dof * (dof + 1) // 2 + LANE_FIELDS * 64 + n_links * 12)


def ldlt_branch(n):
    """which routine ldlt_solve_any takes for a system of n unknowns"""
    return "rows8" if n <= 8 else "rows13" if n <= 13 else "rows16" if n <= 16 else "wave"


class Link:
    """one link: parent = index in the structure's list (-1: the root); body: None (body-less), True (a body of its own,
    no images) or the index of a rendered body; tracked: the body carries modalities; place: where a TRACK case puts
    the link (see TrackCase)"""

    def __init__(self, parent, free=ROT_Z, body=None, tracked=None, joint=None, body2joint=None, fixed_body2joint=True,
                 place=None):
        self.parent, self.free, self.body = parent, tuple(free), body
        self.tracked = (body is not None and body is not True) if tracked is None else tracked
        self.joint = np.eye(4) if joint is None else joint
        self.body2joint = np.eye(4) if body2joint is None else body2joint
        self.fixed_body2joint = fixed_body2joint
        self.place = place

    @property
    def dof(self):
        return sum(self.free)


# ---- builders ---------------------------------------------------------------------------------------------------------
def chain(frees, bodies=None):
    """serial chain: link i hangs on link i - 1"""
    bodies = bodies if bodies is not None else [None] * len(frees)
    return [Link(i - 1, f, body=b, place=b if isinstance(b, int) and b is not True else None)
            for i, (f, b) in enumerate(zip(frees, bodies))]


def star(root_free, child_frees, bodies=None):
    """a root with every other link as its child"""
    bodies = bodies if bodies is not None else [None] * (1 + len(child_frees))
    links = [Link(-1, root_free, body=bodies[0], place=0 if bodies[0] is not None else None)]
    for f, b in zip(child_frees, bodies[1:]):
        links.append(Link(0, f, body=b, place=b if isinstance(b, int) and b is not True else None))
    return links


def pad(links, at, n, free):
    """n body-less links of `free` directions appended, one behind the other, to link `at` (free = FIXED: dof 0, they add
    links only; FREE: six unknowns each, which nothing but the Tikhonov diagonal holds)"""
    links = list(links)
    for _ in range(n):
        links.append(Link(at, free))
        at = len(links) - 1
    return links


def fixed_root(links):
    links = list(links)
    r = links[0]
    links[0] = Link(-1, FIXED, body=r.body, tracked=r.tracked, place=r.place)
    return links


class Structure:
    def __init__(self, links, constraints=(), tikhonov=TIKHONOV):
        self.links, self.constraints, self.tikhonov = list(links), list(constraints), tuple(tikhonov)
        assert self.links[0].parent == -1 and all(0 <= l.parent < i for i, l in enumerate(self.links) if i)
        self.children = [[j for j, l in enumerate(self.links) if l.parent == i] for i in range(len(self.links))]
        self.order = []  # depth-first, children in the order of their creation: the order of the stacked link sums

        def visit(i):
            self.order.append(i)
            for c in self.children[i]:
                visit(c)
        visit(0)
        self.first = [0] * len(self.links)  # first_jacobian_index (optimizer.cpp:237-250)
        dof = 0
        for i in self.order:
            self.first[i] = dof
            dof += self.links[i].dof
        self.n_links, self.dof = len(self.links), dof
        self.n_rows = sum(sum(c["directions"]) for c in self.constraints if c["kind"] == "hard")
        self.size = self.dof + self.n_rows
        self.open = not self.constraints
        self.work_floats = tree_work_floats(self.n_links, self.dof, self.n_rows)
        self.block_floats = ((self.n_links * LINK_DEV_BYTES + 3) // 4 + self.n_links * 42 + self.dof * self.dof + self.dof +
                             self.work_floats + 3) // 4 * 4  # UploadTreeTables: ctx->tree_block_floats
        self.leaf = self.order[-1]


def constraint(kind, link1, link2, directions, body12joint1=None, body22joint2=None, **kw):
    return dict(kind=kind, link1=link1, link2=link2, directions=tuple(directions),
                body12joint1=np.eye(4) if body12joint1 is None else body12joint1,
                body22joint2=np.eye(4) if body22joint2 is None else body22joint2, kw=kw)


class Built:
    """a structure behind one context: links[i] / bodies[i] belong to Structure.links[i]"""


def build(api, st, bodies=None):
    out = Built()
    out.structure = st
    out.bodies = bodies if bodies is not None else [host.Body(api, np.eye(4)) if l.body is not None else None
                                                    for l in st.links]
    out.links = []
    for l, body in zip(st.links, out.bodies):
        out.links.append(host.Link(api, body=body, parent=out.links[l.parent] if l.parent >= 0 else None,
                                   body2joint_pose=l.body2joint, joint2parent_pose=l.joint, free_directions=l.free,
                                   fixed_body2joint_pose=l.fixed_body2joint))
    out.optimizer = host.Optimizer(api, root_link=out.links[0], tikhonov_parameter_rotation=st.tikhonov[0],
                                   tikhonov_parameter_translation=st.tikhonov[1])
    for c in st.constraints:
        cls = host.Constraint if c["kind"] == "hard" else host.SoftConstraint
        cls(api, out.optimizer, out.links[c["link1"]], out.links[c["link2"]], body12joint1_pose=c["body12joint1"],
            body22joint2_pose=c["body22joint2"], constraint_directions=c["directions"], **c["kw"])
    return out


def link_state(built):
    """[link][link2world, joint2parent, body2joint], the structure's links in the order of its list"""
    return np.stack([np.stack([l.link2world_pose(), l.joint2parent_pose(), l.body2joint_pose()]) for l in built.links])


# ---- the solve alone: injected link sums ------------------------------------------------------------------------------
def _small_pose(rng, rot=0.3, trans=0.05):
    return syn.make_pose(syn.rot_vec(rng.uniform(-rot, rot, 3)), rng.uniform(-trans, trans, 3))


def _posed(links, seed, body2joint=False):
    """seeded joint poses for the links of a solve case; body2joint: non-trivial body2joint poses too, on every second
    link a free one (Link::UpdatePoses then moves body2joint, not joint2parent)"""
    rng = np.random.default_rng(seed)
    for i, l in enumerate(links):
        if l.parent >= 0:
            l.joint = _small_pose(rng)
        if body2joint:
            l.body2joint = _small_pose(rng, 0.2, 0.02)
            l.fixed_body2joint = i % 2 == 0
    return links


def _closed(links, seed, kind, directions, **kw):
    """the loop closed between the root and the last link: the closing joint's two images a small pose apart"""
    st = Structure(links)
    rel = np.eye(4)
    path, i = [], st.n_links - 1
    while i > 0:
        path.append(i)
        i = links[i].parent
    for i in reversed(path):
        rel = rel @ links[i].joint.astype(np.float64) @ links[i].body2joint.astype(np.float64)
    d = _small_pose(np.random.default_rng(seed + 1000), 0.05, 0.01)
    return constraint(kind, 0, st.n_links - 1, directions, body22joint2=np.linalg.inv(d) @ rel, **kw)


# The injected systems are indefinite (Tikhonov diagonal minus J^T H J with H positive) and now and then close to
# singular: the cases below take their sums from another seed, chosen so that after one round the oracle and the float64
# restatement of tests/test_structure_edge_cases.py differ by less than 6e-7 in every pose entry while every structure
# moves by more than 2e-3 (first seed + 1000 j that does; s stays 10^U(0, 6))
_SUMS_SEEDS = {"chain-n6": 1006, "chain-n8": 3008, "chain-n9": 1009, "chain-n13": 1013, "chain-n14": 2014, "chain-n15": 3015,
               "chain-n16": 1016, "chain-n17": 1017, "chain-n32": 5032, "chain-n64": 3064, "chain-n65": 2065,
               "fixed-root-n1": 5101, "fixed-root-n9": 1109, "work-arrays-n27": 1227, "work-arrays-n28": 6228,
               "joints-6dof-n18": 2306, "star-5x4dof": 1310, "mixed-n7-n18-n40": 39600, "mixed-n7-global-scratch": 4610}


class SolveCase:
    """structures: the context's structures; modes[k]: how structure k's link sums are made -- "random" (the scheme of
    `sums`), "zero" (every H = 0), "coupled-ties" (the root's H off its diagonal only, the others 0), "leaf-zero" (the last link's
    H = 0), "nan" (one NaN in one link's g) or "nan-h" (one NaN
    on the diagonal of one link's H: the system's diagonal holds NaNs);
    moves[k]: must the oracle move structure k; entry: "sums" (Begin / inject / End, links_solve_sums_kernel) or "plain"
    (CalculateOptimization: links_project_kernel + links_solve_kernel, nothing injected)"""

    ROUNDS = 3

    def __init__(self, id, group, structures, modes=None, moves=None, entry="sums", seed=0, s_max=6.0):
        self.id, self.group, self.structures, self.entry, self.seed, self.s_max = id, group, list(structures), entry, seed, s_max
        self.modes = list(modes) if modes is not None else ["random"] * len(self.structures)
        self.moves = list(moves) if moves is not None else [True] * len(self.structures)
        self.sums_seed = _SUMS_SEEDS.get(id, seed)
        self.n_links = sum(st.n_links for st in self.structures)
        self.sizes = [st.size for st in self.structures]
        self.work_in_lds = max(st.work_floats for st in self.structures) <= LDS_WORK_LIMIT_FLOATS
        # compared with the float64 restatement: open trees with the default Tikhonov parameters and finite sums
        self.f64 = entry == "sums" and all(st.open and st.tikhonov == TIKHONOV for st in self.structures) and \
            all(m in ("random", "zero", "coupled-ties") for m in self.modes)
        rng = np.random.default_rng(seed + 77)
        self.root_poses = [syn.make_pose(syn.rot_vec(rng.uniform(-1, 1, 3)), rng.uniform(-0.3, 0.3, 3)) for _ in self.structures]

    def __repr__(self):
        return self.id

    def sums(self, round_index):
        """the stacked link sums of one round: per link g (6) then H (36), the links of a structure depth first.
        H = (M M^T) s with M 6 x 8 normal and s = 10^U(0, s_max) (magnitudes that differ from link to link: the diagonal
        pivoting really permutes), g = 10 normal"""
        rng = np.random.default_rng([self.sums_seed, round_index, 4242])
        out = []
        for st, mode in zip(self.structures, self.modes):
            for k, i in enumerate(st.order):
                m = rng.normal(size=(6, 8))
                h = (m @ m.T) * 10.0 ** rng.uniform(0.0, self.s_max)
                h = (0.5 * (h + h.T)).astype(np.float32)
                g = (10.0 * rng.normal(size=6)).astype(np.float32)
                if mode == "zero" or (mode == "leaf-zero" and i == st.leaf) or (mode == "coupled-ties" and k > 0):
                    h[:] = 0.0
                if mode == "coupled-ties" and k == 0:
                    h = (100.0 * rng.normal(size=(6, 6))).astype(np.float32)
                    h = np.tril(h, -1) + np.tril(h, -1).T
                if mode == "nan" and k == st.n_links // 2:
                    g[3] = np.nan
                if mode == "nan-h" and k == st.n_links // 2:
                    h[2, 2] = np.nan
                out += [g, h.reshape(-1)]
        return np.concatenate(out).astype(np.float32)


def _one_dof_chain(n, root=FREE, seed=0, leaf=None, **kw):
    """a root and one-dof joints (rotations and translations in turn), then the leaf if one is given, that give a system of
    n unknowns"""
    k = n - sum(root) - (sum(leaf) if leaf else 0)
    frees = [root] + [tuple(1 if d == (j * 5) % 6 else 0 for d in range(6)) for j in range(k)] + ([leaf] if leaf else [])
    return Structure(_posed(chain(frees), seed), **kw)


def lds_limit_pair():
    """(N, N + 1): the one-dof chains under a fixed body-less root whose work arrays are the last to fit the LDS and the
    first that go to global scratch"""
    n = 1
    while tree_work_floats(n + 2, n + 1, 0) <= LDS_WORK_LIMIT_FLOATS:
        n += 1
    return n, n + 1


def _solve_cases():
    cases = []
    add = cases.append
    for n in (6, 7, 8, 9, 13, 14, 15, 16, 17, 32, 64, 65):
        add(SolveCase("chain-n%d" % n, "size", [_one_dof_chain(n, seed=n)], seed=n))
    for n in (1, 7, 8, 9):
        st = _one_dof_chain(n + 6, seed=100 + n)
        add(SolveCase("fixed-root-n%d" % n, "size", [Structure(fixed_root(st.links))], seed=100 + n))
    for n in lds_limit_pair():
        add(SolveCase("work-arrays-n%d" % n, "lds-limit", [_one_dof_chain(n, root=FIXED, seed=200 + n)], seed=200 + n))
    for d in (4, 5, 6):
        st = Structure(_posed(chain([FREE, JOINT[d], JOINT[d]]), 300 + d))
        add(SolveCase("joints-%ddof-n%d" % (d, st.size), "joint-shape", [st], seed=300 + d))
    add(SolveCase("star-5x4dof", "joint-shape", [Structure(_posed(star(FREE, [JOINT[4]] * 5), 310))], seed=310))
    add(SolveCase("body2joint-n16", "joint-shape",
                  [Structure(_posed(chain([FREE, JOINT[5], JOINT[5]], bodies=[True, None, True]), 320, body2joint=True))],
                  seed=320))
    rows = {1: (0, 0, 0, 1, 0, 0), 3: (0, 0, 0, 1, 1, 1), 6: FREE}
    for n, r, seed in ((8, 1, 408), (9, 1, 409), (13, 3, 423), (14, 3, 414), (16, 6, 416), (17, 6, 417)):
        links = _posed(chain([FREE] + [ROT_Z if j % 2 else (0, 1, 0, 0, 0, 0) for j in range(n - r - 6)]), seed)
        st = Structure(links, [_closed(links, seed, "hard", rows[r])])
        assert st.size == n
        add(SolveCase("closed-%drows-n%d" % (r, n), "constraint", [st], seed=seed))
    links = _posed(chain([FREE] + [ROT_Z if j % 2 else (0, 1, 0, 0, 0, 0) for j in range(8)]), 450)
    add(SolveCase("soft-n14", "constraint", [Structure(links, [_closed(links, 450, "soft", FREE)])], seed=450))
    # degenerate pivots
    for n in (8, 13, 16):  # H = 0: the diagonal holds the two Tikhonov values only -- equal values, the step-by-step selection
        add(SolveCase("ties-n%d" % n, "degenerate", [_one_dof_chain(n, seed=500 + n)], modes=["zero"], seed=500 + n))
    # ... and the same diagonal with entries beside it, where the order of equal pivots changes the rounding: the free
    # root's H has a zero diagonal (its Jacobian is the identity: the system's diagonal stays the Tikhonov vector), the
    # other links' H = 0
    for n in (8, 13, 16):
        add(SolveCase("coupled-ties-n%d" % n, "degenerate", [_one_dof_chain(n, seed=540 + n)], modes=["coupled-ties"],
                      seed=540 + n))
    add(SolveCase("all-zero-n8", "degenerate", [_one_dof_chain(8, seed=510, tikhonov=(0.0, 0.0))], modes=["zero"],
                  moves=[False], seed=510))
    # (a leaf of four free directions: four zero columns, the first zero pivot has rows below it)
    add(SolveCase("zero-pivot-n11", "degenerate", [_one_dof_chain(11, seed=520, leaf=JOINT[4], tikhonov=(0.0, 0.0))],
                  modes=["leaf-zero"], seed=520))
    add(SolveCase("zero-pivot-n18", "degenerate", [_one_dof_chain(18, seed=521, leaf=JOINT[4], tikhonov=(0.0, 0.0))],
                  modes=["leaf-zero"], seed=521))
    add(SolveCase("nan-beside-healthy", "degenerate", [_one_dof_chain(9, seed=530), _one_dof_chain(9, seed=531)],
                  modes=["nan", "random"], moves=[False, True], seed=530))
    add(SolveCase("nan-n17-beside-healthy", "degenerate", [_one_dof_chain(17, seed=532), _one_dof_chain(8, seed=533)],
                  modes=["nan", "random"], moves=[False, True], seed=532))
    add(SolveCase("nan-hessian-beside-healthy", "degenerate", [_one_dof_chain(13, seed=534), _one_dof_chain(16, seed=535)],
                  modes=["nan-h", "random"], moves=[False, True], seed=534))
    # several structures of different sizes in one launch: the grid is the structures, the LDS the largest one's
    add(SolveCase("mixed-n7-n18-n40", "mixed",
                  [_one_dof_chain(7, seed=600), Structure(_posed(chain([FREE, FREE, FREE]), 601)),
                   Structure(_posed(chain([FREE] * 6 + [JOINT[4]]), 602))], seed=600))
    n_lds, n_global = lds_limit_pair()
    add(SolveCase("mixed-n7-global-scratch", "mixed", [_one_dof_chain(7, seed=610), _one_dof_chain(n_global, root=FIXED, seed=611)],
                  seed=610))
    # the same code entered through CalculateOptimization: nothing injected, hard constraints drive the structure
    for n, r in ((9, 1), (14, 3), (17, 6)):
        links = _posed(chain([FREE] + [ROT_Z if j % 2 else (0, 1, 0, 0, 0, 0) for j in range(n - r - 6)]), 700 + n)
        add(SolveCase("plain-closed-n%d" % n, "plain", [Structure(links, [_closed(links, 700 + n, "hard", rows[r])])],
                      entry="plain", seed=700 + n))
    return cases


SOLVE_CASES = _solve_cases()


def write_host(ptr, n, data):
    np.ctypeslib.as_array(ptr, shape=(n,))[:] = data


class SolveRun:
    """start: the links' state after CalculateConsistentPoses; states[r]: after round r (both: per structure, link_state)"""


def solve_run(api, case, write=write_host):
    built = [build(api, st) for st in case.structures]
    for b, pose in zip(built, case.root_poses):
        b.links[0].set_link2world_pose(pose)
    tracker = host.Tracker(api, 1, 1)
    assert tracker.CalculateConsistentPoses()
    out = SolveRun()
    out.built = built
    out.start = [link_state(b) for b in built]
    out.states = []
    for r in range(case.ROUNDS):
        if case.entry == "plain":
            assert tracker.CalculateOptimization(0, 0, 0)
        else:
            ptr, n = tracker.CalculateOptimizationBegin()
            assert n == 42 * case.n_links
            write(ptr, n, case.sums(r))
            assert tracker.CalculateOptimizationEnd()
        out.states.append([link_state(b) for b in built])
    return out


# ---- the fused tree kernels: structures tracked with images -----------------------------------------------------------
TREE_VARIABLES = ("M3T_HIP_NO_TREE_SPLIT", "M3T_HIP_TREE_PARTS", "M3T_HIP_NO_TREE_FUSION", "M3T_HIP_NO_TREE_SEGMENTS")
# launch shape -> (overrides, kind, the largest part count the shape allows)
SHAPES = {
    "auto": ({}, "fused", 8),
    "parts2": ({"M3T_HIP_TREE_PARTS": "2"}, "fused", 2),
    "parts1": ({"M3T_HIP_TREE_PARTS": "1"}, "fused", 1),
    "unfused": ({"M3T_HIP_NO_TREE_FUSION": "1"}, "unfused", 0),
    "segment": ({}, "segment", 0),  # a reduce callback that leaves the sums as they are: world size 1, no RCCL
}
N_FRAMES = 2


def _r4(x):
    return (x + 3) // 4 * 4


def _chain_pitch(n):
    slots = (n + 23) // 24 * 24  # m3t_kernels.hip: chain_slots (kChainBlock 24), chain_pitch
    return slots if (slots // 4) & 1 else slots + 4


def tree_step_lds(region_params, depth_params, block_floats):
    """TreeStepLds over ComputeLayout: bytes of LDS of one workgroup of a tracking_step_tree_* kernel; None where the
    pair table is staged in LDS (layout.off_hist >= 0: no tree kernel)"""
    nl = region_params["n_lines_max"]
    ns = max(9, region_params["function_length"] + region_params["distribution_length"] - 1)
    bins3 = region_params["n_histogram_bins"] ** 3
    if bins3 * 8 <= 32 * 1024:
        return None
    block = _r4(1024 + 31 * nl)
    off = block + 3 * nl * ns
    rows_end = block + 27 * _chain_pitch(nl)
    if depth_params is not None:
        rows_end += 27 * _chain_pitch(depth_params["n_points_max"])
    off = _r4(max(off, rows_end))
    if depth_params is not None:
        off += 13 * depth_params["n_points_max"]
    lds_track = off * 4
    counts_in_lds = 1024 * 4 + bins3 * 4 <= CU_LDS_BYTES
    front = max(lds_track, 1024 * 4 + bins3 * 4) if counts_in_lds else lds_track
    return (front + 15) // 16 * 16 + block_floats * 4


class TrackCase:
    """structures: lists of Link rows whose `body` is the index of a rendered body (bench_chain.chain_inputs: three bodies,
    a free root and two revolute joints) and whose `place` says where the link starts: an int j = where body j starts, None
    = 1 cm along x behind its parent, a function of the bodies' start poses = that pose.  The joints of a case need not be
    the rendered ones: the criterion is the oracle."""

    def __init__(self, id, group, structures, region=None, tracker=(7, 2), inputs_args=None, depth=False, edit=None,
                 moves=None, empty=(), tracks=True):
        self.id, self.group, self.structures = id, group, list(structures)
        self.depth = depth
        base = dict(syn.YCB_REGION_PARAMS, n_histogram_bins=32) if depth else dict(syn.RBOT_REGION_PARAMS, measure_occlusions=0)
        self.region_params = dict(base, **(region or {}))
        self.depth_params = dict(syn.YCB_DEPTH_PARAMS) if depth else None
        self.n_corr, self.n_update = tracker
        self.inputs_args = dict(inputs_args or {})
        self.edit = edit
        self.n_bodies = 2 if depth else 3
        # (structure, link) of every link with a body / with modalities, in the order the library meets them
        self.body_links = [(s, i) for s, st in enumerate(self.structures) for i in st.order if st.links[i].body is not None]
        self.tracked_links = [(s, i) for s, i in self.body_links if self.structures[s].links[i].tracked]
        self.moves = list(moves) if moves is not None else [True] * len(self.body_links)
        self.empty = tuple(empty)  # indices into tracked_links: no valid line, histograms stay as started
        self.tracks = tracks       # the bodies stay within 5 degrees / 5 cm of the rendered motion
        self.constrained = any(st.constraints for st in self.structures)
        self.newton_steps = self.n_corr * self.n_update
        self.lds = tree_step_lds(self.region_params, self.depth_params, max(st.block_floats for st in self.structures))
        self.expect = _expect(self)

    def __repr__(self):
        return self.id


def _expect(case):
    """{shape: (kernel, [workgroups, parts, threads] or None)}; kernel "": per-sub-step launches, no shape of their own"""
    rp = case.region_params
    n_tracked = len(case.tracked_links)
    fused_possible = all(st.n_links <= FUSED_MAX_LINKS and st.size <= FUSED_MAX_SIZE for st in case.structures)
    one_launch = fused_possible and case.lds is not None and case.lds <= CU_LDS_BYTES
    elements = max(rp["n_lines_max"], case.depth_params["n_points_max"] if case.depth else 1)
    split_ok = not case.constrained and case.n_corr < 64 and rp["n_histogram_bins"] >= 4

    def parts(limit):  # m3t_step_plan.h, SplitParts (every workgroup resident: 256 CUs, one workgroup each)
        for p in (16, 8, 4, 2):
            if p <= limit and (elements + p - 1) // p <= 256 // p and n_tracked * p <= COMPUTE_CUS:
                return p
        return 0

    suffix = "constrained_" if case.constrained else ""
    out = {}
    for shape, (_, kind, limit) in SHAPES.items():
        if kind == "unfused" or not one_launch or (kind == "fused" and case.newton_steps >= 63):
            out[shape] = ("", None)
        elif kind == "segment":
            out[shape] = ("tracking_step_tree_segment_%skernel" % suffix, [n_tracked, 1, 512])
        else:
            p = parts(limit) if split_ok else 0
            out[shape] = ("tracking_step_tree_split_kernel", [n_tracked, p, 512]) if p >= 2 else \
                ("tracking_step_tree_%skernel" % suffix, [n_tracked, 1, 512])
    return out


_inputs = {}


def inputs_of(case):
    """(inputs, joints, gt) of the case, generated once per process and argument set; runs do not change them"""
    key = (case.depth, repr(sorted(case.inputs_args.items())), case.edit.__name__ if case.edit else None)
    if key in _inputs:
        return _inputs[key]
    if case.depth:  # two Region + Depth bodies on a revolute joint (tests/test_gpu_multibody.py, DepthChain's frames)
        inputs = scenes.Inputs(2, 1, n_divides=2, with_depth=True)
        rng = np.random.default_rng(11)
        joints = [syn.make_pose(syn.rot_vec([0.3, -0.2, 0.1]), [0.16, 0.02, 0.0])]
        pose_a, angle, gt = inputs.gt[0][0].copy(), 0.2, []
        color, depth = [[], []], [[], []]
        for k in range(N_FRAMES):
            pose_a = syn.perturb_pose(pose_a, rng, rot_deg=0.7, trans=0.002)
            angle += rng.uniform(-0.03, 0.03)
            poses = [pose_a.copy(), pose_a @ joints[0] @ syn.make_pose(syn.rot_vec([0, 0, angle]), [0, 0, 0])]
            gt.append((poses, np.array([angle])))
            for i in range(2):
                c, d = inputs.scenes[i].render(poses[i])
                color[i].append(c)
                depth[i].append(d)
        inputs = scenes.subset(inputs, [0, 1])
        inputs.color, inputs.depth = color, depth
    else:
        args = case.inputs_args
        shim = types.SimpleNamespace(Inputs=lambda *a, **kw: scenes.Inputs(*a, **dict(kw, **args)))
        inputs, joints, gt = bench_chain.chain_inputs(shim, syn, 3, N_FRAMES, 2)
    if case.edit is not None:
        inputs = scenes.subset(inputs, list(range(inputs.n_objects)))
        inputs.depth = [list(frames) for frames in inputs.depth]
        case.edit(inputs)
    _inputs[key] = (inputs, joints, gt)
    return _inputs[key]


def start_poses(joints, gt):
    """where the rendered bodies start: the root half a degree and a millimetre off, the angles 0.01 rad off
    (tests/test_gpu_multibody.py, test_eight_body_chain_matches_the_oracle)"""
    poses = [syn.perturb_pose(gt[0][0][0], np.random.default_rng(5), rot_deg=0.5, trans=0.001).astype(np.float64)]
    for j, joint in enumerate(joints):
        poses.append(poses[-1] @ joint @ syn.make_pose(syn.rot_vec([0, 0, gt[0][1][j] + 0.01]), [0, 0, 0]))
    return poses


class Tracked:
    """a TrackCase behind one context"""

    def __init__(self, api, case, inputs, joints, gt):
        self.api, self.case = api, case
        body_start = start_poses(joints, gt)
        rmodels = [host.RegionModel(api, data_points=m[0], orientations=m[1], contour_lengths=m[2]) for m in inputs.region_models]
        dmodels = [host.DepthModel(api, data_points=m[0], orientations=m[1], surface_areas=m[2])
                   for m in inputs.depth_models] if case.depth else []
        self.built, self.feeds, self.region = [], [], []
        for st in case.structures:
            nominal = [None] * st.n_links
            for i, l in enumerate(st.links):  # (parents come first in the list)
                if callable(l.place):
                    nominal[i] = np.asarray(l.place(body_start), np.float64)
                elif l.place is not None:
                    nominal[i] = body_start[l.place]
                else:
                    step = np.eye(4)
                    step[0, 3] = 0.01
                    nominal[i] = nominal[l.parent] @ step
                if l.parent >= 0:
                    l.joint = (np.linalg.inv(nominal[l.parent]) @ nominal[i]).astype(np.float32)
            for c in st.constraints:  # (a loop closes where the bodies start)
                if isinstance(c["body12joint1"], _Closing):
                    c["body12joint1"] = c["body12joint1"].resolve(body_start)
            bodies = [host.Body(api, np.eye(4)) if l.body is not None else None for l in st.links]
            b = build(api, st, bodies)
            for i in st.order:
                l = st.links[i]
                if l.body is None:
                    continue
                cam = host.ColorCamera(api, **inputs.intr)
                dcam = host.DepthCamera(api, depth_scale=inputs.depth_scale, **inputs.intr) if case.depth else None
                self.feeds.append((l.body, cam, dcam))
                if not l.tracked:
                    continue
                r = host.RegionModality(api, bodies[i], cam, rmodels[inputs.model_of[l.body]], depth_camera=dcam,
                                        **case.region_params)
                b.links[i].AddModality(r)
                self.region.append(r)
                if case.depth:
                    b.links[i].AddModality(host.DepthModality(api, bodies[i], dcam, dmodels[inputs.model_of[l.body]],
                                                              **case.depth_params))
            b.links[0].set_link2world_pose(nominal[0])
            self.built.append(b)
        self.tracker = host.Tracker(api, case.n_corr, case.n_update)
        assert self.tracker.CalculateConsistentPoses()
        self.inputs = inputs

    def upload(self, k):
        for body, cam, dcam in self.feeds:
            cam.UpdateImage(self.inputs.color[body][k])
            if dcam is not None:
                dcam.UpdateImage(self.inputs.depth[body][k])

    def state(self):
        """body2world of every body, then joint2parent of every link but the roots"""
        out = [self.built[s].bodies[i].body2world_pose() for s, i in self.case.body_links]
        for b in self.built:
            out += [b.links[i].joint2parent_pose() for i in b.structure.order[1:]]
        return np.stack(out)

    def histograms(self):
        return [r.histograms() for r in self.region]


class TrackRun:
    """start / states[k]: Tracked.state() before the first and after frame k; hist_start / hist: the histograms after
    StartModalities and after the last frame; from the oracle the valid lines of every RegionModality, from the device the
    kernel and launch shape of every frame and the number of reductions"""


def track_run(api, case, device=False, segment=False):
    inputs, joints, gt = inputs_of(case)
    t = Tracked(api, case, inputs, joints, gt)
    out = TrackRun()
    keep = None
    if segment:
        keep = util.pkg._capi.REDUCE_FN(lambda user, buffer, count, stream: 0)
        api.call("comm_set_reduce_callback", C.cast(keep, C.c_void_p), None)
    out.start = t.state()
    t.upload(0)
    assert t.tracker.StartModalities(0)
    out.hist_start = t.histograms()
    out.states, out.kernels, out.shapes = [], [], []
    for k in range(N_FRAMES):
        t.upload(k)
        assert t.tracker.ExecuteTrackingStep(k), (case.id, k)
        out.states.append(t.state())  # (the read-back also waits for the step)
        if device:
            out.kernels.append(fused_edges.kernel_of(api))
            out.shapes.append(fused_edges.shape_of(api))
    out.hist = t.histograms()
    if device:
        count = C.c_longlong(-1)
        api.call("comm_get_allreduce_count", C.byref(count))
        out.reductions = count.value
    else:
        out.n_lines = [len(r.data_lines()) for r in t.region]
    if segment:
        api.call("comm_set_reduce_callback", None, None)
    out.gt = gt
    return out


def oracle_track_run(case):
    return track_run(util.open_oracle(), case)


# ---- the table of tracked cases ---------------------------------------------------------------------------------------
def _bodies_chain(d):
    """the three rendered bodies on joints of d free directions"""
    return chain([FREE, JOINT[d], JOINT[d]], bodies=[0, 1, 2])


def _off_screen(body_start):
    pose = body_start[2].copy()
    pose[0, 3] += 3.0
    return pose


def _zero_depth_of_the_leaf(inputs):
    inputs.depth[1] = [np.zeros_like(f) for f in inputs.depth[1]]


def lds_limit_padding(region_params):
    """(k, k + 1): the numbers of six-dof body-less links behind the one-dof chain of three bodies whose structure copy is
    the last to fit the tree kernels' LDS and the first that does not"""
    k = 0
    while True:
        st = Structure(pad(_bodies_chain(1), 2, k + 1, FREE))
        lds = tree_step_lds(region_params, None, st.block_floats)
        if lds > CU_LDS_BYTES or st.size > FUSED_MAX_SIZE or st.n_links > FUSED_MAX_LINKS:
            return k, k + 1
        k += 1


_BINS64 = dict(n_histogram_bins=64)  # (the count table of 64 bins is not kept in LDS: room for a larger structure copy)


def _track_cases():
    cases = []
    add = cases.append
    for d in (1, 4, 5, 6):
        st = Structure(_bodies_chain(d))
        add(TrackCase("joints-%ddof-n%d" % (d, st.size), "solve-size", [st]))
    # the limits of the one-launch kernels' structure code: links, system size, LDS.  The padding adds Tikhonov rows only:
    # the poses are those of the plain chain
    for k in (13, 14):
        add(TrackCase("links-%d" % (3 + k), "limits", [Structure(pad(_bodies_chain(1), 2, k, FIXED))], region=_BINS64))
    add(TrackCase("links-16-bins32", "limits", [Structure(pad(_bodies_chain(1), 2, 13, FIXED))]))
    add(TrackCase("plain-bins64", "limits", [Structure(_bodies_chain(1))], region=_BINS64))
    for k in lds_limit_padding(dict(syn.RBOT_REGION_PARAMS, **_BINS64)):
        st = Structure(pad(_bodies_chain(1), 2, k, FREE))
        add(TrackCase("padded-n%d" % st.size, "limits", [st], region=_BINS64))
    st = Structure(pad(pad(_bodies_chain(1), 2, 9, FREE), 11, 2, ROT_Z))
    add(TrackCase("padded-n%d" % st.size, "limits", [st], region=_BINS64))
    st = Structure(pad(pad(_bodies_chain(1), 2, 9, FREE), 11, 3, ROT_Z))
    add(TrackCase("padded-n%d" % st.size, "limits", [st], region=_BINS64))
    # the host's rules
    add(TrackCase("star", "host-rules", [Structure(star(FREE, [ROT_Z, ROT_Z], bodies=[0, 1, 2]))]))
    add(TrackCase("newton-31x2", "host-rules", [Structure(_bodies_chain(1))], tracker=(31, 2)))
    add(TrackCase("newton-9x7", "host-rules", [Structure(_bodies_chain(1))], tracker=(9, 7)))
    add(TrackCase("newton-1x1", "host-rules", [Structure(_bodies_chain(1))], tracker=(1, 1)))
    add(TrackCase("newton-3x3", "host-rules", [Structure(_bodies_chain(1))], tracker=(3, 3)))
    for b in (2, 16, 64):
        add(TrackCase("bins-%d" % b, "host-rules", [Structure(_bodies_chain(1))], region=dict(n_histogram_bins=b)))
    add(TrackCase("points300-lines257", "host-rules", [Structure(_bodies_chain(1))], region=dict(n_lines_max=257),
                  inputs_args=dict(n_points=300)))
    # topology
    links = _bodies_chain(1)
    links[1].tracked = False
    add(TrackCase("middle-untracked", "topology", [Structure(links)]))
    links = _bodies_chain(1)
    links[1] = Link(0, ROT_Z, body=None, place=1)
    add(TrackCase("middle-bodyless", "topology", [Structure(links)]))
    add(TrackCase("two-structures", "topology", [Structure(_bodies_chain(6)),
                                                 Structure(star(FREE, [ROT_Z, ROT_Z], bodies=[0, 1, 2]))]))
    # geometry
    links = _bodies_chain(1)
    links[2].place = _off_screen
    add(TrackCase("leaf-off-screen", "geometry", [Structure(links)], empty=(2,), tracks=False))
    add(TrackCase("image-333x251", "geometry", [Structure(_bodies_chain(1))], inputs_args=dict(intr=fused_edges._ODD_IMAGE)))
    # parameters of the correspondence search, on the one-dof chain
    for s in ([1], [9, 7, 5, 2], [10, 3]):
        add(TrackCase("scales-" + "-".join(map(str, s)), "parameters", [Structure(_bodies_chain(1))],
                      region=dict(scales=s, standard_deviations=[15.0] * len(s)), tracker=(len(s), 2)))
    for fl, dl in ((6, 10), (16, 16)):
        add(TrackCase("lengths-%d-%d" % (fl, dl), "parameters", [Structure(_bodies_chain(1))],
                      region=dict(function_length=fl, distribution_length=dl, scales=[2, 1], standard_deviations=[7.0, 1.5])))
    # constrained structures: a closed loop A -- B -- C -- A
    c2joint = syn.make_pose(syn.rot_vec([0.1, 0.2, -0.3]), [0.02, 0.03, -0.01])
    for name, d, kind, directions in (("closed-1dof-3rows-n11", 1, "hard", (0, 0, 0, 1, 1, 1)),
                                      ("closed-4dof-3rows-n17", 4, "hard", (0, 0, 0, 1, 1, 1)),
                                      ("closed-5dof-1row-n17", 5, "hard", (0, 0, 0, 1, 0, 0)),
                                      ("soft-1dof", 1, "soft", (0, 0, 0, 1, 1, 1))):
        add(TrackCase(name, "constrained", [Structure(_bodies_chain(d), [
            constraint(kind, 0, 2, directions, body12joint1=_Closing(c2joint), body22joint2=c2joint)])], tracks=False))
    # Region + Depth links
    add(TrackCase("depth-4dof-n10", "depth", [Structure(chain([FREE, JOINT[4]], bodies=[0, 1]))], depth=True, tracker=(4, 2)))
    add(TrackCase("depth-4dof-leaf-zero-depth", "depth", [Structure(chain([FREE, JOINT[4]], bodies=[0, 1]))], depth=True,
                  tracker=(4, 2), edit=_zero_depth_of_the_leaf))
    return cases


class _Closing:
    """body12joint1 of a loop's closing joint, known once the bodies' start poses are: the joint seen from C carried to A"""

    def __init__(self, c2joint):
        self.c2joint = c2joint

    def resolve(self, body_start):
        a_t_c = np.linalg.inv(body_start[0]) @ body_start[2]
        return (self.c2joint @ np.linalg.inv(a_t_c)).astype(np.float32)


TRACK_CASES = _track_cases()
TRACK_PAIRS = [(c, s) for c in TRACK_CASES for s in SHAPES]
