"""gymothelloenv_amd -- MI355X-native vectorised Othello rules engine.

Hot path of omurammm/GymOthelloEnv (othello.py's legal moves, flips,
terminal/score) as HIP kernels for gfx950 behind a C ABI
(include/othello_mi355x.h, library liboth_mi355x.so in this directory).

    VecOthelloEnv            E boards in HBM (the performance path)
    OthelloBaseEnv,          drop-in single-board classes with the
    SimpleOthelloEnv,        reference's constructor / attributes / 4-tuple step
    OthelloEnv
    RandomPolicy, GreedyPolicy, MaxiMinPolicy, MonteCarloPolicy, MCTSPolicy, PUCTPolicy,
    SolverPolicy, SearchPolicy, NetPolicy, NTuplePolicy,
    make_state, undo_state
    default_search_weights   the conventional square weights of VecOthelloEnv.search
    SearchConfig             a search as a player: VecOthelloEnv.play_search, and the
                             opponent of reset_vs / step_vs
    masked_sample, masked_log_prob   policy-head sampling over legal squares
    puct_quantize, PuctLeaves,       the network-guided tree search of VecOthelloEnv.puct_begin /
    uniform_evaluator,               puct_advance / puct_result / puct_search: a network's floats as the
    playout_evaluator                search's integers, its leaves, and two evaluators without a network
    PuctPlay                         one move of self-play on that search's tree (VecOthelloEnv.puct_play:
                                     puct_pick, step, puct_reroot)
    ReplayBatch,                     the replay store of VecOthelloEnv.replay_begin / replay_append /
    symmetry_masks,                  replay_label / replay_gather / replay_sample: a minibatch, masks under a
    symmetry_permutations            board symmetry, and the eight square permutations sigma_s
    DeviceNet, MLPPolicyValue,       the int8 policy-value network evaluated on the device (oth_net_eval): an
    net_features                     evaluator without a float, the float module a learner trains, its inputs
    NetPlayer                        a DeviceNet or a DeviceConvNet as a player: VecOthelloEnv.play_net, and the
                                     opponent of reset_vs / step_vs (argmax of the logits, or a draw from the
                                     priors; oth_play_net for the MLP, oth_play_cnet for the conv net)
    DeviceConvNet, ConvPolicyValue   the int8 residual convolutional network on the device (oth_cnet_eval) and
                                     the float module a learner trains: an evaluator and a player as a DeviceNet is
    RootNoise, dirichlet_table       Dirichlet root noise for self-play, drawn on the device in integers
                                     (VecOthelloEnv.puct_noise; puct_search / puct_play take noise=RootNoise(...))
    NTupleNet, snake_tuples,         the n-tuple network (oth_ntuple_eval, oth_ntuple_update): look-up tables over
    ntuple_evaluator                 small sets of squares that evaluate and learn on the device in integers, the
                                     evaluation of VecOthelloEnv.search_ntuple and an evaluator of puct_search
    NTuplePlayer, TDRows             an NTupleNet as a player: VecOthelloEnv.play_ntuple (with the TD(0) rows of
                                     its plies from the same launch), the opponent of reset_vs / step_vs, and
                                     NTupleNet.td_play, a TD round in two calls (oth_play_ntuple,
                                     oth_ntuple_update_masked)
"""
from ._lib import LIB_PATH, OthelloLibError, load  # noqa: F401

BLACK_DISK, NO_DISK, WHITE_DISK = -1, 0, 1


def __getattr__(name):
    # lazy: importing the package must not touch the GPU (build() runs on CPU hosts)
    if name in ("VecOthelloEnv", "legal_moves", "default_search_weights", "SearchConfig", "PuctLeaves",
                "PuctPlay", "puct_quantize", "uniform_evaluator", "playout_evaluator", "ReplayBatch",
                "symmetry_masks", "symmetry_permutations"):
        from . import vec_env
        return getattr(vec_env, name)
    if name in ("DeviceNet", "MLPPolicyValue", "net_features", "NetPlayer"):
        from . import net
        return getattr(net, name)
    if name in ("DeviceConvNet", "ConvPolicyValue"):
        from . import cnet
        return getattr(cnet, name)
    if name in ("RootNoise", "dirichlet_table"):
        from . import noise
        return getattr(noise, name)
    if name in ("NTupleNet", "snake_tuples", "ntuple_evaluator", "NTuplePlayer", "TDRows"):
        from . import ntuple
        return getattr(ntuple, name)
    if name in ("OthelloBaseEnv", "SimpleOthelloEnv", "OthelloEnv"):
        from . import othello
        return getattr(othello, name)
    if name in ("RandomPolicy", "GreedyPolicy", "MaxiMinPolicy", "MonteCarloPolicy", "MCTSPolicy",
                "PUCTPolicy", "SolverPolicy", "SearchPolicy", "NetPolicy", "NTuplePolicy"):
        from . import policies
        return getattr(policies, name)
    if name in ("masked_sample", "masked_log_prob"):
        from . import masked
        return getattr(masked, name)
    if name in ("make_state", "undo_state"):
        from . import util
        return getattr(util, name)
    raise AttributeError(name)
