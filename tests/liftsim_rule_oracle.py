"""Host restatement of the reference's rule-based dispatcher (metagym/liftsim/tests/rule_benchmark/dispatcher.py,
Rule_dispatcher.policy): a MansionState in, the flat action list [target, direction] * E out.

TEST INFRASTRUCTURE, written from the dispatcher's behaviour and pinned to runs of the unmodified one in
tests/golden/liftsim_rule.npz. The rule, as the device function `rule_policy` (liftsim.hip) also states it:

Every hall call (floor, side) has a holder (an elevator, or nobody) and the holder's priority. The elevators wait in a
first-in first-out line, 0 .. E-1 at the start; an elevator that loses its call to a better one joins the line again.
The elevator at the front of the line bids by its Direction:
  * moving up (down): on the up (down) calls at or beyond its floor, by nearness, +5 (capped at 0) for a floor it has
    already reserved, -5 when its Velocity is below EPSILON (signed, so every downward mover pays it). The best call
    whose holder it strictly beats is taken with indicator +1 (also when moving down); the loser's action goes back to
    (0, 1). With no such call it takes the highest (lowest) unheld call of the other side, writing a priority without
    comparing one; this never displaces anybody.
  * Direction 0: the nearest call of either side it strictly beats, up calls scanned first; the loser joins the line
    but KEEPS its action, which it still has at the end if its next bid finds nothing.
An elevator holds at most one call while it is outside the line and none while inside, so the line never holds more than
E entries; `stats` (a dict) counts what happened, under the names the fixture's event counts use.
"""
EPSILON = 1.0e-2
HUGE = 1.0e8
UP, DOWN = 0, 1


def policy(state, stats=None):
    els = state.ElevatorStates
    E = len(els)
    calls = (list(state.RequiringUpwardFloors), list(state.RequiringDownwardFloors))
    holder = ({f: -1 for f in calls[UP]}, {f: -1 for f in calls[DOWN]})
    prio = ({f: -HUGE for f in calls[UP]}, {f: -HUGE for f in calls[DOWN]})
    action = [[0, 1] for _ in range(E)]
    line = list(range(E))
    taken = longest = 0
    ev = stats if stats is not None else {}

    def count(name):
        ev[name] = ev.get(name, 0) + 1
    while line:
        longest = max(longest, len(line))
        k = line.pop(0)
        taken += 1
        me = els[k]
        if me.Direction != 0:
            side = UP if me.Direction > 0 else DOWN
            best, best_p = -1, -HUGE
            for f in calls[side]:
                if (side == UP and f < me.Floor - EPSILON) or (side == DOWN and f > me.Floor + EPSILON):
                    continue
                p = me.Floor - f if side == UP else -me.Floor + f
                if f in me.ReservedTargetFloors:
                    p = min(0.0, p + 5.0)
                    count("reserved_bonus")
                if me.Velocity < EPSILON:
                    p -= 5.0
                if p > prio[side][f] and p > best_p:
                    best, best_p = f, p
            if best > 0:
                action[k] = [best, 1]
                count("assign_up" if side == UP else "assign_down")
                loser = holder[side][best]
                if loser >= 0:
                    action[loser] = [0, 1]
                    line.append(loser)
                    count("displace_up" if side == UP else "displace_down")
                holder[side][best], prio[side][best] = k, best_p
                continue
            other = 1 - side
            free = [f for f in calls[other] if holder[other][f] < 0]
            if free:
                f = max(free) if side == UP else min(free)
                action[k] = [f, -1 if side == UP else 1]
                count("fallback_up" if side == UP else "fallback_down")
                holder[other][f] = k
                prio[other][f] = (-me.Floor - EPSILON + f) if side == UP else (me.Floor + EPSILON - f)
        else:
            best, best_p, best_side = -1, -HUGE, UP
            for side in (UP, DOWN):
                for f in calls[side]:
                    p = -abs(f - me.Floor)
                    if p > prio[side][f] and p > best_p:
                        best, best_p, best_side = f, p, side
            if best > 0:
                action[k] = [best, 1 if best_side == UP else -1]
                count("assign_zero")
                loser = holder[best_side][best]
                if loser >= 0:
                    line.append(loser)
                    count("displace_zero_up" if best_side == UP else "displace_zero_down")
                holder[best_side][best], prio[best_side][best] = k, best_p
    count("calls")
    if taken > E:
        count("calls_with_displacement")
    ev["max_taken"] = max(ev.get("max_taken", 0), taken)
    ev["max_line"] = max(ev.get("max_line", 0), longest)
    return [x for a in action for x in a]
