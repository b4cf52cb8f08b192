"""Rule sets for the join tests (test_join_model.py, test_gpu_join.py): a
synthetic set with every edge the join kernels branch on planted in it, and
plain NodeIDs-only sets for the degenerate sizes."""
import numpy as np

from cronsun_amd import synth
from cronsun_amd.engine import RulesIn
from patch_common import World

EDGE_RULES = 15      # rules edge_rules plants after the synthetic ones
GROUP_CAP = 100      # members kept of a synthetic group (bounds nnz; still > 64)
SYNTH_MIN_NODES = 16  # synth.multi_rule_jobs draws groups of >= 2 distinct nodes


def edge_rules(N, R, keys, seed, rules_per_job=(1, 4)):
    """R rules over N nodes on top of synth.multi_rule_jobs(..., n_nodes=N):
    the first R - EDGE_RULES rules are synthetic (groups cut to GROUP_CAP
    members; for N < 16 drawn over 16 nodes and folded mod N, which also
    repeats ids inside lists), then seven planted jobs:

      A  one rule on nodes 0 and N-1 (in every mode), ex = N, N+31, 2^31-1
      B  two rules on the all-nodes group (listed descending); the second also
         names the missing group
      C  one rule of 130 NodeIDs with repeats, the group of the top 200 nodes,
         and 100 excludes (some >= N)
      D  a paused job of two rules with nodes
      E  two rules with no node: only the missing group, and nothing at all
      F  a chain of six rules of one Cmd key (with keys) over overlapping node
         lists, the fourth excluded on part of its list, the third on a group
      G  one rule naming a group of 100 members (N < 100: of at most 8 ids)

    Returns (RulesIn, info): info names the planted rules and groups."""
    assert R >= EDGE_RULES and N >= 1
    rng = np.random.default_rng(seed)
    M = max(N, SYNTH_MIN_NODES)
    n_syn = R - EDGE_RULES
    rin = synth.multi_rule_jobs(n_syn // rules_per_job[0] + 1, rules_per_job, n_nodes=M, seed=seed,
                                key_choices=keys)
    w = World(rin)
    # the first n_syn rules (the last job may lose rules; jobs stay contiguous)
    w.rule_job, w.nids, w.gids, w.ex = w.rule_job[:n_syn], w.nids[:n_syn], w.gids[:n_syn], w.ex[:n_syn]
    if w.rule_key is not None:
        w.rule_key = w.rule_key[:n_syn]
    w.job_pause = w.job_pause[:(w.rule_job[-1] + 1) if n_syn else 0]
    w.n_nodes = N
    w.groups = [(g[:GROUP_CAP] % N).astype(np.int32) for g in w.groups]
    w.nids = [(x % N).astype(np.int32) for x in w.nids]
    G0 = len(w.groups)
    # one synthetic group of more than 64 members whatever the draw gave
    # (N < 100: at most 8 distinct ids, repeated)
    w.groups[0] = (rng.choice(N, GROUP_CAP, replace=False) if N >= GROUP_CAP
                   else rng.integers(0, min(N, 8), GROUP_CAP)).astype(np.int32)
    w.group_exists[0] = 1
    w.group_exists[1] = 0  # a synthetic group goes missing, rules naming it stay
    g_all, g_top, g_missing = G0, G0 + 1, G0 + 2
    w.groups += [np.arange(N - 1, -1, -1, dtype=np.int32),
                 np.arange(max(N - 200, 0), N, dtype=np.int32),
                 np.arange(min(N, 5), dtype=np.int32)]
    w.group_exists += [1, 1, 0]
    top = 2**31 - 1
    many = rng.integers(0, N, 130)
    many[1] = many[0]
    many[129] = many[64]
    ex100 = np.concatenate([rng.integers(0, N, 90), [N, N + 31, top], rng.integers(N, N + 1000, 7)])
    pool = rng.integers(0, N, 30)
    chain = []
    for i in range(6):
        nids = rng.choice(pool, 20)
        gids = [g_top] if i == 2 else []
        ex = nids[:8] if i == 3 else rng.choice(pool, 2)
        chain.append((nids, gids, ex, 0))
    k = (lambda i: i % keys) if keys else (lambda i: 0)
    first = w.n_rules
    w.add_job([([0, N - 1], [], [N, N + 31, top], k(0))])
    w.add_job([([], [g_all], [N + 31], k(0)), ([N // 2], [g_all, g_missing], [N // 3, top], k(1))])
    w.add_job([(many, [g_top], ex100, k(1))])
    w.add_job([([0, N // 2], [g_top], [], k(0)), ([N - 1], [], [], k(0))], pause=1)
    w.add_job([([], [g_missing], [0], k(0)), ([], [], [], k(1))])
    w.add_job(chain)
    w.add_job([([], [0], [N], k(0))])
    assert w.n_rules == R
    out = w.pack()
    info = dict(first=first, all_nodes=(first + 1, first + 2), many=first + 3, paused=(first + 4, first + 5),
                empty=(first + 6, first + 7), chain=tuple(range(first + 8, first + 14)), big_group=first + 14,
                g_all=g_all, g_top=g_top, g_missing=g_missing)
    # nnz <= the distinct ids the rules list: keeps the host model within
    # seconds at 524288 nodes
    sizes = np.array([len(np.unique(g)) for g in w.groups]) * out.group_exists[:out.n_groups]
    listed = np.diff(out.nid_off[:R + 1])
    np.add.at(listed, np.repeat(np.arange(R), np.diff(out.gid_off[:R + 1])), sizes[out.gids[:out.gid_off[R]]])
    assert np.minimum(listed, N).sum() <= 2 * N + 150000, listed.sum()
    return out, info


def nid_rules(N, lists, pause=None):
    """One job per rule, NodeIDs only."""
    lists = [np.asarray(x, dtype=np.int32) for x in lists]
    nid_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return nid_rules_csr(N, nid_off, np.concatenate(lists) if len(lists) and nid_off[-1] else np.zeros(0, np.int32),
                         pause)


def nid_rules_csr(N, nid_off, nids, pause=None):
    """nid_rules from the lists as one CSR (nid_off [R+1], nids): no Python
    loop over the rules, for sets of 10^6 rules."""
    R = len(nid_off) - 1
    zero = np.zeros(R + 1, dtype=np.int64)
    return RulesIn(N, 0, R, R, group_off=np.zeros(1, np.int64), group_nodes=np.zeros(0, np.int32),
                   group_exists=np.zeros(0, np.uint8), rule_job=np.arange(R, dtype=np.int32),
                   nid_off=np.ascontiguousarray(nid_off, dtype=np.int64),
                   nids=np.ascontiguousarray(nids, dtype=np.int32),
                   gid_off=zero, gids=np.zeros(0, np.int32), ex_off=zero, ex=np.zeros(0, np.int32),
                   job_pause=np.zeros(R, np.uint8) if pause is None else np.asarray(pause, np.uint8))
