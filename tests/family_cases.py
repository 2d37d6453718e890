"""Cases shared by the search families' tests at every board size and on arbitrary
positions: the host builds' per-size cases (tests/test_*_host.py), the device's
(tests/test_gpu_family_sizes.py) and the arbitrary-position table with its
references (tests/test_family_census.py, tests/test_gpu_family_property.py).

The kernels are templates over the board size N, and three kinds of their code
change with N or with W = ceil(N*N / 64): the playouts' flip engine (one word,
two words with a table in LDS, three or four words), the `if constexpr (W ...)`
branches of the playouts and the tree searches, and the observation writers
(N*N % 4).  So every family runs at every N from 4 to 16 somewhere: the sizes
below are the ones the families' own test files leave out.

Every reference here is one of the existing plain-Python ones; this module only
chooses shapes, builds positions, caches results and states, on the references
alone, what a case is there to reach."""
import numpy as np

import mcts_ref as mr
import playout_ref as pr
import puct_batch_ref as pb
import puct_play_ref as pp
import puct_ref as pf
import search_ref as sh
import solve_ref as sr
from oracle import oracle

ALL_SIZES = list(range(4, 17))
# one word: 5, 7; two: 9, 11; three: 12, 13; four with a partly used last word: 14, 15
NEW_SIZES = [5, 7, 9, 11, 12, 13, 14, 15]
NEW_SIZES_SOLVE = [n for n in NEW_SIZES if n != 5]  # solve, search and play-search run 5 x 5 in their own files


# ------------------------------------------------------------ the cases of every size
def solve_max_e(n):
    """The most empty squares of a size's solve batch: what the plain minimax reference values in a second or two."""
    return 9 if n <= 8 else 7 if n <= 11 else 5


SEARCH_WSET, SEARCH_DEPTHS = "random", (1, 2, 3)    # the weight set with mobility != 0
PLAY_PLIES = {5: 8, 7: 6, 9: 6, 11: 4, 12: 3, 13: 3, 14: 3, 15: 3}  # the move-choice run's plies (test_gpu_play_search)


def mcts_case(n, full=False):
    """(n, E, I, R, C, T) of mcts_ref; full: T = N*N, the tree fills."""
    return (n, 9, 40, 3, 256, n * n if full else 4096)


# simulations of the plain search: 40, more where the smallest boards need them for a selection decided by the
# lowest-square rule (puct_ref.check_case; found on the reference: 5 x 5 has none below 100, 7 x 7 none at 40, the
# full 7 x 7 tree none below 200)
PUCT_SIMS = {5: 100, 7: 60}
PUCT_SIMS_FULL = {7: 200, 13: 40}


def puct_case(n, full=False):
    """(n, E, sims, C, T) of puct_ref."""
    return (n, 9, PUCT_SIMS_FULL[n], 320, n * n) if full else (n, 9, PUCT_SIMS.get(n, 40), 320, 4096)


def play_case(n):
    """(n, E, S, M, C, T) of puct_play_ref: 9 boards, 3 moves of 20 simulations; on 5 x 5 twelve boards and on 9 x 9
    16 simulations, where the nine-board, twenty-simulation game has no kept child that no selection had made
    (puct_play_ref.check_case)."""
    E, S = {5: (12, 20), 9: (9, 16)}.get(n, (9, 20))
    return (n, E, S, 3, 320, 4096)


def batch_case(n):
    """(n, E, sims, C, T, K) of puct_batch_ref."""
    return (n, 9, 40, 320, 4096, 4)


MCTS_FULL, PUCT_FULL = (7, 12), (7, 13)
BATCH_WIDE = (12, 70, 40, 320, 4096, 3)   # more boards than a wave at a three-word stride, K no power of two
OBS_SIZES = (5, 7, 9, 13)                 # N*N % 4 != 0 with one, two and three words


def tree_census(boards):
    """(pass children, deepest path) of reference Boards (puct_ref.Board and its subclasses), from the nodes themselves:
    the batch reference's selection does not count them."""
    passes, depth = 0, 0
    for b in boards:
        for i, nd in b.nodes.items():
            if i == 0 or not nd.made:
                continue
            parent = b.nodes[nd.parent]
            passes += (not nd.term) and nd.white_to_move == parent.white_to_move
            depth = max(depth, nd.depth)
    return passes, depth


_BATCH_RUNS = {}


def batch_run(c):
    """(positions, Run, (pass children, depth)) of a batch case, computed once and never changed."""
    if c not in _BATCH_RUNS:
        n, E, sims, C, T, K = c
        s = mr.positions(n, E)
        search = pb.Search(s, C, T, K)
        run = pb.Run.__new__(pb.Run)
        run.leaves, run.mid = [search.leaves()], {}
        while run.leaves[-1][0].any():  # pb.Run's loop, keeping the boards for the census
            if len(run.leaves) in (1, 3):
                run.mid[len(run.leaves) - 1] = (search.result(), search.picks())
            _, boards, meta, _ = run.leaves[-1]
            priors, values = pf.hash_eval(boards, meta, search.nn)
            search.advance(priors, values, sims)
            run.leaves.append(search.leaves())
            assert len(run.leaves) <= sims + 2
        run.outputs, run.counters = search.result(), search.counters
        run.root_visits = np.array([b.nodes[0].v for b in search.boards])
        _BATCH_RUNS[c] = (s, run, tree_census(search.boards))
        pb._CACHE.setdefault(c, (s, run))  # puct_batch_ref.case(c) is this run
    s, run, census = _BATCH_RUNS[c]
    return s.copy(), run, census


def check_batch_case(c, run, census):
    """puct_batch_ref.check_case, and what it does not look at: a pass child made, depth >= 3."""
    pb.check_case(c, run)
    assert census[0] > 0, "no child was made after a pass"
    assert census[1] >= 3


def check_play_case(c, game):
    """puct_play_ref.check_case, and: a kept board whose kept child had been expanded (it brings nodes along), a board
    not kept."""
    pp.check_case(c, game)
    assert any(((mv["kept"] == 1) & (mv["used"] > 1)).any() for mv in game.moves), "no kept child had been expanded"
    assert any((mv["kept"] == 0).any() for mv in game.moves)


# ------------------------------------------------------------ arbitrary positions
ARB_E = 25  # boards per example: not a multiple of 8 (the tree searches' groups), several boards a wave


def pack(mask, n):
    W = oracle.nwords(n)
    out = np.zeros((mask.shape[0], W), dtype=np.uint64)
    for a in range(n * n):
        out[:, a // 64] |= mask[:, a].astype(np.uint64) << np.uint64(a % 64)
    return out


def arbitrary(n, E, seed, db, dw):
    """E arbitrary positions, the generator of test_gpu_property._positions with E a parameter: each square black with
    probability db, white with dw, else empty; the side to move drawn per board; possible_moves as the oracle computes
    them for that side.  No board is flagged terminated, whoever can move."""
    rng = np.random.RandomState(seed)
    u = rng.rand(E, n * n)
    black, white = u < db, (u >= db) & (u < db + dw)
    B, Wt = pack(black, n), pack(white, n)
    turn = np.where(rng.rand(E) < 0.5, 1, -1)  # +1: white to move
    tw = (turn == 1)[:, None]
    s = oracle.State(n, E)
    s.boards[:] = np.concatenate([B, Wt], 1)
    s.meta[:] = oracle.meta_from(turn)
    s.legal[:] = oracle.legal(n, np.where(tw, Wt, B), np.where(tw, B, Wt))
    return s


def kinds(s):
    """(mover has a move, opponent has a move) per board, from the discs alone."""
    W = s.W
    tw = ((s.meta & 1) != 0)[:, None]
    B, Wt = s.boards[:, :W], s.boards[:, W:]
    mine = oracle.legal(s.n, np.where(tw, Wt, B), np.where(tw, B, Wt)).any(1)
    theirs = oracle.legal(s.n, np.where(tw, B, Wt), np.where(tw, Wt, B)).any(1)
    return mine, theirs


def narrowed(s):
    """s with the stored mask of every third board that has two moves or more narrowed to every second legal square
    (not the lowest), and emptied on one more such board.  Subsets of the legal mask only: a wider mask is not defined."""
    nn = s.n * s.n
    t = s.copy()
    wide = [e for e in range(s.E) if pr.legal_bool(s.legal[e], nn).sum() >= 2]
    for e in wide[::3]:
        t.legal[e] = sr.mask_words(np.flatnonzero(pr.legal_bool(s.legal[e], nn))[1::2], s.n)
    if len(wide) >= 2:
        t.legal[wide[1]] = 0
    return t


BANDS = ("near_full", "lopsided", "half_empty", "full")


def densities(n, band):
    """(db, dw) of a band.  near_full: about four empty squares a board -- 0.9 on the small boards, 0.97 on the large
    ones -- so that the tree searches reach game ends within 30 simulations and the solver's boards are within its
    size's empties; lopsided: the mover is often stuck while the opponent has a move, and passes repeat; full: nobody
    can move although no board is flagged terminated."""
    if band == "near_full":
        t = min(0.97, max(0.9, 1.0 - 4.0 / (n * n)))
        return (t / 2, t / 2)
    return {"lopsided": (0.02, 0.9), "half_empty": (0.3, 0.3), "full": (0.5, 0.5)}[band]


TABLE = [(n, 1000 * n + k, ) + densities(n, band) for n in ALL_SIZES for k, band in enumerate(BANDS)]
SOLVED_BANDS = (0, 3)  # oth_solve and oth_search run on the near-full and the full band (rows k of a size)


def row_id(row):
    return "n%d-seed%d-b%.3f-w%.3f" % row


def row_state(row):
    n, seed, db, dw = row
    return narrowed(arbitrary(n, ARB_E, seed, db, min(dw, 1.0 - db)))


# the shapes of the families on arbitrary positions
# test_gpu_playouts' key: a 64-bit seed, an id that wraps inside the batch, the high counter word in use
ARB_KEY = dict(seed=0x1234567887654321, id_key=12345, id_base=2 ** 32 - 9, counter=2 ** 40 + 3)
ARB_PLAYOUTS = ((False, 3), (True, 2))     # (per_move, R)
ARB_MCTS = (30, 2, 256, 4096)              # I, R, C, T
ARB_PUCT = (30, 320, 4096)                 # sims, C, T
ARB_BATCH = (30, 320, 4096, 4)             # sims, C, T, K
ARB_GAME = (12, 3, 320, 4096)              # S, M, C, T
ARB_SEARCH_DEPTH = 2

_ARB = {}


def _cached(key, make):
    if key not in _ARB:
        _ARB[key] = make()
    return _ARB[key]


def arb_playouts(row, per_move, R):
    k = ARB_KEY
    return _cached(("playouts", row, per_move, R),
                   lambda: pr.replay(row_state(row), per_move, R, k["seed"], k["id_key"], k["id_base"], k["counter"]))


def arb_mcts(row):
    I, R, C, T = ARB_MCTS
    return _cached(("mcts", row),
                   lambda: mr.search(row_state(row), I, R, C, T, mr.SEED, mr.ID_KEY, mr.ID_BASE, mr.COUNTER))


def arb_puct(row):
    sims, C, T = ARB_PUCT
    return _cached(("puct", row), lambda: pf.Run(row_state(row), sims, C, T))


def arb_batch(row):
    sims, C, T, K = ARB_BATCH
    return _cached(("batch", row), lambda: pb.Run(row_state(row), sims, C, T, K))


def arb_game(row):
    S, M, C, T = ARB_GAME
    return _cached(("game", row), lambda: pp.Game(row_state(row), S, M, C, T))


def arb_solve(row):
    return _cached(("solve", row), lambda: sr.solve(row_state(row), max_empties=solve_max_e(row[0])))


def arb_search(row):
    ws = sh.weight_sets(row[0])[SEARCH_WSET]
    return _cached(("search", row), lambda: (sh.search(row_state(row), ARB_SEARCH_DEPTH, *ws), ws))
