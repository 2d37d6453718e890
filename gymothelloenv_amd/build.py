"""Build liboth_mi355x.so in-tree with hipcc for gfx950 (no JIT cache: the .so
travels with the repo snapshot to the GPU box).

The kernels are templates over the board size N; csrc/kernels_n.hip is
compiled once per N (-DOTH_N=4..16) in parallel, csrc/play_rand_n.hip (the
fused random-play kernels, its own scheduler flags) once per N = 4..11, csrc/playouts_n.hip
(oth_playouts), csrc/solve_n.hip (oth_solve), csrc/search_n.hip (oth_search),
csrc/play_search_n.hip (oth_play_search, oth_reset_vs_search, oth_step_vs_search),
csrc/play_net_n.hip (oth_play_net, oth_reset_vs_net, oth_step_vs_net: the network as a player),
csrc/play_cnet_n.hip (oth_play_cnet, oth_reset_vs_cnet, oth_step_vs_cnet: the conv net as a player) and
csrc/mcts_n.hip (oth_mcts) and csrc/puct_n.hip (oth_puct_begin, oth_puct_advance, oth_puct_result, oth_puct_pick,
oth_puct_reroot) and csrc/replay_n.hip (oth_replay_begin, oth_replay_append, oth_replay_label, oth_replay_counts,
oth_replay_gather, oth_replay_sample, oth_symmetry_masks) and csrc/ntuple_n.hip (oth_ntuple_eval,
oth_ntuple_update, oth_search_ntuple: the n-tuple network) and csrc/play_ntuple_n.hip (oth_play_ntuple,
oth_reset_vs_ntuple, oth_step_vs_ntuple: the n-tuple network as a player) once per N,
csrc/net.hip (oth_net_eval: the int8 network on the matrix cores), csrc/cnet.hip (oth_cnet_eval: the int8
residual convolutional network on the matrix cores) and csrc/noise.hip (oth_puct_noise: Dirichlet root noise in
integers) once for every N,
csrc/capi.hip holds the C ABI, and the objects are linked into one shared library.

Reproducibility: objects go to a fixed directory (`_objs/`, git-ignored) so the
compiler's per-TU ids (derived from the input path and options) are the same on
every build, and the library embeds the SHA-256 of its sources and flags
(`oth_version()` reports it, `embedded_hash()` reads it from the file).  The
loader refuses a library whose embedded hash is not the hash of the sources in
the tree, so a binary that ran on the GPU box is provably built from HEAD."""
import concurrent.futures
import hashlib
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
SIZES = list(range(4, 17))
SOURCES = ("capi.hip", "kernels_n.hip", "play_rand_n.hip", "masked.hip", "device.hpp", "launch.hpp", "bitboard.hpp",
           "masked.hpp", "ply.hpp", "sample_step.hpp", "maximin_wave.hpp", "playouts_n.hip", "playouts.hpp",
           "tables.hpp", "state.hpp", "engines.hpp", "policy.hpp", "play.hpp", "vs.hpp", "observe.hpp", "solve_n.hip",
           "solve.hpp", "root_tasks.hpp", "search_n.hip", "search.hpp", "play_search_n.hip", "play_search.hpp",
           "mcts_n.hip", "mcts.hpp", "puct_n.hip", "puct.hpp", "replay_n.hip", "replay.hpp", "net.hip", "net.hpp",
           "noise.hip", "noise.hpp", "net_dev.hpp", "play_owner.hpp", "play_net_n.hip", "play_net.hpp", "cnet.hip",
           "cnet.hpp", "cnet_dev.hpp", "play_cnet_n.hip", "play_cnet.hpp", "ntuple_n.hip", "ntuple.hpp",
           "play_ntuple_n.hip", "play_ntuple.hpp")
PLAY_SIZES = list(range(4, 12))  # k_play_rand (one-word boards) and k_play_rand_w (two-word boards)
# play_rand_n.hip: the max-ILP machine scheduler (one wave per SIMD: latency hidden by the schedule
# counts, occupancy does not); the rest of the library keeps the default scheduler
PLAY_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# playouts_n.hip (oth_playouts), every board size: a unit of its own so that it can carry scheduler flags
# of its own.  Several waves per SIMD share its latency, and max-ilp measured within the spread of two
# runs at 65,536 boards x 8, -1.5 % at 1,024 boards x 64 per move and -4 % on one board x 65,536
# (profiles/playouts_sched_ab.json): it keeps the default scheduler
PLAYOUT_FLAGS = []
DEPS = [os.path.join(CSRC, f) for f in SOURCES] + [os.path.join(ROOT, "include", "othello_mi355x.h")]
OUT = os.path.join(HERE, "liboth_mi355x.so")
OBJDIR = os.path.join(HERE, "_objs")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("OTH_OFFLOAD_ARCH", "gfx950")
BASE_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-pass-failed"]
_HASH_RE = re.compile(rb"oth-src-sha256:([0-9a-f]{64})")


def play_flags(out=OUT):
    """play_rand_n.hip's scheduler flags: PLAY_FLAGS for the shipped library;
    OTH_PLAY_FLAGS replaces them for the tools' A/B variants (out != OUT) only."""
    if out != OUT and os.environ.get("OTH_PLAY_FLAGS") is not None:
        return os.environ["OTH_PLAY_FLAGS"].split()
    return list(PLAY_FLAGS)


def source_hash(extra_flags=(), out=OUT):
    """SHA-256 over the library's sources (name + bytes) and its build flags."""
    h = hashlib.sha256()
    for p in DEPS:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    h.update(" ".join([ARCH] + BASE_FLAGS + play_flags(out) + PLAYOUT_FLAGS + list(extra_flags)).encode())
    return h.hexdigest()


def embedded_hash(path=OUT):
    """The source hash a built library carries (None if absent or unreadable)."""
    try:
        with open(path, "rb") as f:
            m = _HASH_RE.search(f.read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def needs_build(out=OUT, extra_flags=()):
    return embedded_hash(out) != source_hash(extra_flags, out)


def _jobs():
    n = os.cpu_count() or 4
    cap = int(os.environ.get("MAX_JOBS", "16"))
    return max(1, min(n, cap, len(SIZES) + 2))


def build(force=False, verbose=True, extra_flags=(), out=OUT, jobs=None, only_sizes=None, only_units=None):
    """only_sizes (A/B variants of the tools, never the shipped library): compile the
    per-N units of these board sizes only and link the other sizes' objects of the
    main build (which must exist) -- a variant of one size in a fraction of the time.
    only_units (the same, by source): compile only the units of these sources
    (("puct_n",): every board size of puct_n.hip) and capi.hip, link the rest."""
    if not force and not needs_build(out, extra_flags):
        return out
    assert (only_sizes is None and only_units is None) or out != OUT, "the shipped library is always built whole"
    digest = source_hash(extra_flags, out)
    objdir = OBJDIR if out == OUT else os.path.join(OBJDIR, os.path.splitext(os.path.basename(out))[0])
    shutil.rmtree(objdir, ignore_errors=True)
    os.makedirs(objdir)
    base = [HIPCC, "--offload-arch=%s" % ARCH] + BASE_FLAGS + ["-I", os.path.join(ROOT, "include")] + list(extra_flags)
    units = [(os.path.join(CSRC, "capi.hip"), os.path.join(objdir, "capi.o"), ['-DOTH_SRC_HASH="%s"' % digest]),
             (os.path.join(CSRC, "masked.hip"), os.path.join(objdir, "masked.o"), []),
             (os.path.join(CSRC, "net.hip"), os.path.join(objdir, "net.o"), []),
             (os.path.join(CSRC, "cnet.hip"), os.path.join(objdir, "cnet.o"), []),
             (os.path.join(CSRC, "noise.hip"), os.path.join(objdir, "noise.o"), [])]
    units += [(os.path.join(CSRC, "kernels_n.hip"), os.path.join(objdir, "kernels_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "play_rand_n.hip"), os.path.join(objdir, "play_rand_n%d.o" % n),
               ["-DOTH_N=%d" % n] + play_flags(out)) for n in PLAY_SIZES]
    units += [(os.path.join(CSRC, "playouts_n.hip"), os.path.join(objdir, "playouts_n%d.o" % n),
               ["-DOTH_N=%d" % n] + PLAYOUT_FLAGS) for n in SIZES]
    units += [(os.path.join(CSRC, "solve_n.hip"), os.path.join(objdir, "solve_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "search_n.hip"), os.path.join(objdir, "search_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "play_search_n.hip"), os.path.join(objdir, "play_search_n%d.o" % n),
               ["-DOTH_N=%d" % n]) for n in SIZES]
    units += [(os.path.join(CSRC, "play_net_n.hip"), os.path.join(objdir, "play_net_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "play_cnet_n.hip"), os.path.join(objdir, "play_cnet_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "mcts_n.hip"), os.path.join(objdir, "mcts_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "puct_n.hip"), os.path.join(objdir, "puct_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "replay_n.hip"), os.path.join(objdir, "replay_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "ntuple_n.hip"), os.path.join(objdir, "ntuple_n%d.o" % n), ["-DOTH_N=%d" % n])
              for n in SIZES]
    units += [(os.path.join(CSRC, "play_ntuple_n.hip"), os.path.join(objdir, "play_ntuple_n%d.o" % n),
               ["-DOTH_N=%d" % n]) for n in SIZES]

    def compile_one(u):
        src, obj, defs = u
        cmd = base + defs + ["-c", "-o", obj, src]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stdout))
        return obj

    if verbose:
        print("hipcc %s -> %s (%d units, src %s)" % (" ".join(base[1:]), out, len(units), digest[:16]), flush=True)
    reuse = []
    if only_units is not None:
        keep = {os.path.basename(u[1]) for u in units
                if os.path.basename(u[1]) == "capi.o" or os.path.basename(u[1]).startswith(tuple(only_units))}
    if only_sizes is not None:
        keep = {"capi.o", "masked.o", "net.o", "cnet.o", "noise.o"} | {"kernels_n%d.o" % n for n in only_sizes} | {"play_rand_n%d.o" % n
                                                                                   for n in only_sizes} | {
            "playouts_n%d.o" % n for n in only_sizes} | {"solve_n%d.o" % n for n in only_sizes} | {
            "search_n%d.o" % n for n in only_sizes} | {"play_search_n%d.o" % n for n in only_sizes} | {"play_net_n%d.o" % n for n in only_sizes} | {"play_cnet_n%d.o" % n for n in only_sizes} | {
            "mcts_n%d.o" % n for n in only_sizes} | {"puct_n%d.o" % n for n in only_sizes} | {
            "replay_n%d.o" % n for n in only_sizes} | {"ntuple_n%d.o" % n for n in only_sizes} | {
            "play_ntuple_n%d.o" % n for n in only_sizes}
    if only_sizes is not None or only_units is not None:
        reuse = [os.path.join(OBJDIR, os.path.basename(u[1])) for u in units if os.path.basename(u[1]) not in keep]
        units = [u for u in units if os.path.basename(u[1]) in keep]
        missing = [o for o in reuse if not os.path.exists(o)]
        if missing:
            raise RuntimeError("only_sizes / only_units need the main build's objects: %s" % missing[:3])
        if embedded_hash(OUT) != source_hash():  # the reused objects must come from these sources
            raise RuntimeError("only_sizes / only_units reuse the main build's objects: rebuild %s from the current sources "
                               "first" % OUT)
    with concurrent.futures.ThreadPoolExecutor(jobs or _jobs()) as ex:
        objs = list(ex.map(compile_one, units)) + reuse
    subprocess.check_call([HIPCC, "--offload-arch=%s" % ARCH, "-shared", "-o", out + ".tmp"] + objs, cwd=ROOT)
    os.replace(out + ".tmp", out)
    return out


# oth_puct_reroot's one-lane mapping (csrc/puct.hpp OTH_PUCT_REROOT_LANE) as a second library: the
# GPU tests hold both mappings against the reference, tools/probe_puct_play.py times them
REROOT_LANE_FLAGS = ("-DOTH_PUCT_REROOT_LANE=1",)
REROOT_LANE_OUT = os.path.join(HERE, "variants", "liboth_reroot_lane.so")


def build_reroot_lane(verbose=True):
    """The one-lane variant: 14 units of its own on top of the main build's objects where those are
    there and current, else built whole."""
    os.makedirs(os.path.dirname(REROOT_LANE_OUT), exist_ok=True)
    kw = dict(verbose=verbose, extra_flags=REROOT_LANE_FLAGS, out=REROOT_LANE_OUT)
    try:
        return build(only_units=("puct_n",), **kw)
    except RuntimeError as e:
        if "main build's objects" not in str(e):
            raise
        return build(**kw)


# oth_net_eval cut short after a stage (csrc/net.hip OTH_NET_STOP), for tools/probe_net.py's split of the kernel's
# time: never shipped, never loaded by the package
def net_stop_out(stage):
    return os.path.join(HERE, "variants", "liboth_net_stop%d.so" % stage)


def build_net_stop(stage, verbose=True):
    """Two units (net.hip, capi.hip) on top of the main build's objects, which must be there and current."""
    os.makedirs(os.path.join(HERE, "variants"), exist_ok=True)
    return build(only_units=("net",), verbose=verbose, extra_flags=("-DOTH_NET_STOP=%d" % stage,),
                 out=net_stop_out(stage))


if __name__ == "__main__":
    build(force="--force" in sys.argv)
