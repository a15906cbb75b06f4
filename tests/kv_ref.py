"""Restatement of KVStore::execute and ExecutionOrderMonitor::add
(fantoch/src/kvs.rs:53-85, executor/monitor.rs:8-55) in plain Python: a dict
for the store, a list per key for the monitor, applied over an order list.
Values are ids, 0 is None (canonical C15)."""
from fantoch_amd import kv as K


def execute(store, monitor, key, ops, rifl):
    """One partial: ops (op words) on `key`.  Returns its results, one per op."""
    read_only = all(K.op_kind(op) == K.GET for op in ops)  # kvs.rs:61 (an empty partial is read-only)
    if not read_only:  # monitor.rs:22-24
        monitor.setdefault(key, []).append(rifl)
    results = []
    for op in ops:
        kind = K.op_kind(op)
        if kind == K.GET:
            results.append(store.get(key, 0))
        elif kind == K.PUT:  # does not return the previous value
            store[key] = K.op_value(op)
            results.append(0)
        else:
            assert kind == K.DELETE
            results.append(store.pop(key, 0))
    return results


def run(order, keys_of, ops_of):
    """order: arrival rows in execution order; keys_of[a], ops_of[a]: the key
    and the op words of arrival row a.  Returns (results {a: [..]}, store
    {key: value}, monitor {key: [arrival rows]})."""
    store, monitor, results = {}, {}, {}
    for a in order:
        results[a] = execute(store, monitor, keys_of[a], ops_of[a], a)
    return results, store, monitor


def check_stream(res, s, order, keys_of, ops_of):
    """Stream s of a KvResult against the restatement over `order`."""
    results, store, monitor = run(order, keys_of, ops_of)
    assert int(res.err[s]) == 0, (s, int(res.err[s]))
    for a in order:
        want = results[a] + [0] * (res.omax - len(results[a]))
        assert res.results(s, a) == want, (s, a, res.results(s, a), want)
    assert [int(v) for v in res.store[s]] == [store.get(k, 0) for k in range(res.keys)], s
    assert int(res.mon_off[s, 0]) == 0
    assert int(res.mon_off[s, res.keys]) == sum(len(v) for v in monitor.values()), s
    for k in range(res.keys):
        assert K.monitor_rows(res, s, k) == monitor.get(k, []), (s, k)


def first_difference(mon_a, rifl_a, mon_b, rifl_b, keys):
    """check_monitors of two streams: the smallest (key, position) at which
    the per-key sequences of rifl words differ, or None."""
    for k in range(keys):
        a = [rifl_a[x] for x in mon_a.get(k, [])]
        b = [rifl_b[x] for x in mon_b.get(k, [])]
        for i in range(min(len(a), len(b))):
            if a[i] != b[i]:
                return (k, i)
        if len(a) != len(b):
            return (k, min(len(a), len(b)))
    return None
