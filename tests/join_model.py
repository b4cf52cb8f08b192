"""Host model of the rule -> node join (cg_rule_nodes.hip), its node-major
transpose, the fan-out of a due set and the rule set a patch leaves behind.

Plain numpy over sorted id arrays, no call into the library or the oracle:
test_join_model.py pins it to the oracle (O.node_rules over every node,
or_rule_on_node row by row) at the sizes the oracle can walk; test_gpu_join.py
then holds the kernels to it at the node counts where they change path, where
the oracle's rules x nodes walk takes minutes.

Semantics (Job.Cmds, job.go:591-614), per rule r of job j:
  1. the row is empty if job_pause[j];
  2. else NodeIDs plus the members of every GroupID g with 0 <= g < G and
     group_exists[g], kept to 0 <= n < N;
  3. EXCLUDE_RULE: minus ex[r];
  4. EXCLUDE_CUMULATIVE: minus the ex of every rule from the job's first rule
     through r (paused or empty rules still contribute theirs);
  5. with rule_key: minus the step 1-4 set of every later rule of the job
     with r's key (the set after excludes, before that rule's own shadowing).
"""
import numpy as np

EXCLUDE_NONE, EXCLUDE_RULE, EXCLUDE_CUMULATIVE = 0, 1, 2

_EMPTY = np.zeros(0, dtype=np.int64)


def _cat(parts):
    parts = [np.asarray(p, dtype=np.int64) for p in parts if len(p)]
    return np.concatenate(parts) if parts else _EMPTY


def _minus(a, b):
    """The sorted unique ids a without the ids b (any order, repeats allowed)."""
    if a.size == 0 or len(b) == 0:
        return a
    return a[~np.isin(a, b)]


def _job_runs(rule_job, R):
    """(first, end) of every run of consecutive rules with one rule_job."""
    if R == 0:
        return []
    cut = np.flatnonzero(np.diff(rule_job[:R])) + 1
    first = np.concatenate([[0], cut])
    end = np.concatenate([cut, [R]])
    return list(zip(first.tolist(), end.tolist()))


def rule_sets(rin, mode):
    """Per rule, its ascending node ids (int64 arrays) under `mode`."""
    if mode not in (EXCLUDE_NONE, EXCLUDE_RULE, EXCLUDE_CUMULATIVE):
        raise ValueError("bad exclude mode")
    R, G, N = rin.n_rules, rin.n_groups, rin.n_nodes
    members = {}

    def group(g):
        if g not in members:
            members[g] = np.asarray(rin.group_nodes[rin.group_off[g]:rin.group_off[g + 1]], dtype=np.int64)
        return members[g]

    out = [_EMPTY] * R
    for first, end in _job_runs(rin.rule_job, R):
        paused = bool(rin.job_pause[rin.rule_job[first]])
        after_ex, ex_seen = [], []
        for r in range(first, end):
            ex = rin.ex[rin.ex_off[r]:rin.ex_off[r + 1]]
            ex_seen.append(ex)
            if paused:
                after_ex.append(_EMPTY)
                continue
            parts = [rin.nids[rin.nid_off[r]:rin.nid_off[r + 1]]]
            for g in rin.gids[rin.gid_off[r]:rin.gid_off[r + 1]].tolist():
                if 0 <= g < G and rin.group_exists[g]:
                    parts.append(group(g))
            s = np.unique(_cat(parts))
            s = s[(s >= 0) & (s < N)]
            if mode == EXCLUDE_RULE:
                s = _minus(s, ex)
            elif mode == EXCLUDE_CUMULATIVE:
                s = _minus(s, _cat(ex_seen))
            after_ex.append(s)
        for r in range(first, end):
            s = after_ex[r - first]
            if rin.rule_key is not None and s.size:
                later = [after_ex[q - first] for q in range(r + 1, end) if rin.rule_key[q] == rin.rule_key[r]]
                s = _minus(s, _cat(later))
            out[r] = s
    return out


def transpose(rn_off, rn_nodes, N):
    """Stable sort of the rule-major (node, rule) pairs by node:
    (nt_off [N+1], nt_rule), rules ascending within a node."""
    R = len(rn_off) - 1
    pair_rule = np.repeat(np.arange(R, dtype=np.int32), np.diff(rn_off))
    order = np.argsort(rn_nodes, kind="stable")
    nt_off = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rn_nodes, minlength=N)[:N], out=nt_off[1:])
    return nt_off, pair_rule[order]


def join(rin, mode):
    """(rn_off [R+1], rn_nodes, nt_off [N+1], nt_rule): the rule-major CSR
    (nodes ascending within a rule) and its node-major transpose."""
    rows = rule_sets(rin, mode)
    rn_off = np.zeros(rin.n_rules + 1, dtype=np.int64)
    if rows:
        np.cumsum([len(x) for x in rows], out=rn_off[1:])
    rn_nodes = _cat(rows).astype(np.int32)
    nt_off, nt_rule = transpose(rn_off, rn_nodes, rin.n_nodes)
    return rn_off, rn_nodes, nt_off, nt_rule


def due_filter(nt_off, nt_rule, due):
    """The fan-out of a wake: the node-major join restricted to the due slots,
    (node_off, slots).  A due slot that is on no node (or past the rule set)
    lands nowhere."""
    due = np.asarray(list(due), dtype=np.int64)
    size = max(int(nt_rule.max(initial=-1)), int(due.max(initial=-1))) + 1
    is_due = np.zeros(size, dtype=bool)
    is_due[due] = True
    keep = is_due[nt_rule]
    rank = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return rank[nt_off], nt_rule[keep].astype(np.int32)


def patched(rin, patch_rin, slots):
    """The RulesIn a rebind after cg_dispatcher_patch_rules(patch_rin, slots)
    would upload (rule i = slot i): patch rule p in slot slots[p], every other
    slot of rin as it was, a slot past rin's rules that the patch does not
    name a rule without nodes (a job of its own).  Nodes: the larger n_nodes;
    groups: the patch's (it carries the bound numbering).  The patch replaces
    whole jobs, so every job's slots stay consecutive (pack() checks)."""
    from patch_common import World
    w, p = World(rin), World(patch_rin)
    slots = [int(s) for s in slots]
    assert len(slots) == p.n_rules and len(set(slots)) == len(slots) and min(slots, default=0) >= 0
    keyed = w.rule_key is not None or p.rule_key is not None
    if keyed:  # a set without keys: every rule its own
        w.rule_key = list(range(w.n_rules)) if w.rule_key is None else w.rule_key
        p.rule_key = list(range(p.n_rules)) if p.rule_key is None else p.rule_key
    while w.n_rules <= max(slots, default=-1):
        w.add_job([([], [], [], 0)])
    base = len(w.job_pause)
    w.job_pause.extend(p.job_pause)
    for q, s in enumerate(slots):
        w.rule_job[s] = base + p.rule_job[q]
        w.nids[s], w.gids[s], w.ex[s] = p.nids[q], p.gids[q], p.ex[q]
        if keyed:
            w.rule_key[s] = p.rule_key[q]
    w.groups, w.group_exists = p.groups, p.group_exists
    w.n_nodes = max(w.n_nodes, p.n_nodes)
    return w.pack()
