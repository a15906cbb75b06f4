"""FPaxos's SlotExecutor for one stream, restated (fantoch_ps/src/executor/
slot.rs:16-104): pure Python, no library.

A stream is the list of its slots by arrival row; slots are 1-based
(slot.rs:33-34).  The executor starts with next = 1 and nothing waiting.  For
arrival row a with slot s:

  s < next (which covers s == 0; the assert of slot.rs:55) or s waiting (the
  assert of slot.rs:65-66): the stream stops at this row with SLOT.
  otherwise s waits; then, while `next` waits (try_next_slot, slot.rs:89-96):
  it leaves the waiting set, order.append(its arrival row), release[that row]
  = a, next += 1.

A processed row whose command has not executed at the end has release NONE.
execute_at_commit (slot.rs:57-58): every row executes at its own step; next
never moves, so only s == 0 fails.

What the tiers add: a slot above `steps` stops the stream with CAPACITY
everywhere (not at commit); `window` (the LANE tier: 64) stops it with CAPACITY
at a row with s - next >= window.  At a row the checks go: SLOT for s < next,
then the capacity, then SLOT for a slot that waits.

run() returns order (arrival rows), release {row: step or NONE} over the
processed rows, nexec, err, and reach: the largest s - next any row met before
the stream stopped (the failing row's included where it got that far)."""

NONE = 0xFFFFFFFF
SCC_START = 0x80000000
OK, CAPACITY, SLOT = 0, 2, 17


def run(slots, steps, window=None, execute_at_commit=False):
    order, release, err, reach = [], {}, OK, 0
    nxt, waiting = 1, {}
    for a, s in enumerate(slots):
        if execute_at_commit:
            if s == 0:
                err = SLOT
                break
            order.append(a)
            release[a] = a
            continue
        if s < nxt:
            err = SLOT
            break
        reach = max(reach, s - nxt)
        if s > steps or (window is not None and s - nxt >= window):
            err = CAPACITY
            break
        if s in waiting:
            err = SLOT
            break
        waiting[s] = a
        release[a] = NONE
        while nxt in waiting:
            r = waiting.pop(nxt)
            order.append(r)
            release[r] = a
            nxt += 1
    return dict(order=order, release=release, nexec=len(order), err=err, reach=reach)
