"""AggregatePending for one stream, restated (fantoch/src/executor/aggregate.rs
48-87 with CommandResultBuilder, command.rs:232-263): pure Python, no library.

A stream: `order` (arrival rows in execution order, flags already masked off,
nexec of them), `rifl_of` and `count_of` by arrival row (the count already
masked), `process` (0, or the only source byte, rifl >> 24, whose rows are
waited for).  For every order row, with a its arrival row, r its rifl, c its
count (0 when filtered):

  c = 0   nobody waits for this result: head[a] = IGNORED
  c = 1   a whole command: its own head, complete at once; it meets no builder
  c > 1   no live builder for r: one is created, head a, count c (the earlier
          wait_for); a live one: its count must be c, else INVALID_ARG
  then    part[(got, head)] = a, head[a] = head, got += 1; at got == count:
          index[head] = nready, ready.append(head), the builder is removed

A failing row stops the stream: nothing of it or of later rows is recorded.
live_cap: the most builders a tier holds (None: any number); the row that
would create one more stops the stream with CAPACITY."""

IGNORED = 0xFFFFFFFF
MAX_PARTS = 8
OK, INVALID_ARG, CAPACITY, ORDER_OVERFLOW = 0, 1, 2, 8


def run(order, rifl_of, count_of, steps, nexec=None, process=0, live_cap=None):
    nexec = len(order) if nexec is None else nexec
    out = dict(head={}, part={}, index={}, ready=[], err=OK, nopen=0, peak=0)
    if nexec > steps:
        out["err"] = ORDER_OVERFLOW
        return out
    live = {}
    for a in order[:nexec]:
        if a >= steps:
            out["err"] = INVALID_ARG
            break
        r, c = rifl_of[a], count_of[a]
        if process and (r >> 24) != process:
            c = 0
        if c == 0:
            out["head"][a] = IGNORED
            continue
        if c > MAX_PARTS:
            out["err"] = INVALID_ARG
            break
        if c == 1:
            builder = dict(head=a, count=1, got=0)
        elif r in live:
            builder = live[r]
            if builder["count"] != c:
                out["err"] = INVALID_ARG
                break
        else:
            if live_cap is not None and len(live) >= live_cap:
                out["err"] = CAPACITY
                break
            builder = live[r] = dict(head=a, count=c, got=0)
            out["peak"] = max(out["peak"], len(live))
        h = builder["head"]
        out["part"][(builder["got"], h)] = a
        out["head"][a] = h
        builder["got"] += 1
        if builder["got"] == builder["count"]:
            out["index"][h] = len(out["ready"])
            out["ready"].append(h)
            if c > 1:
                del live[r]
    out["nopen"] = len(live)
    return out
