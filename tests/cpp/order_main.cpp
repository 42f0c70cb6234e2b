// order_main.cpp — the stream order of a handle (csrc/halo_order.h) on the host: every ordering rule as a happens-before statement, without a GPU.
// The API the unit is instantiated with models HIP's stream semantics with one vector clock per stream: work queued on a stream ticks that stream's
// component and keeps a snapshot, record copies the stream's clock into the event, wait joins the event's clock into the stream's (an event never
// recorded: nothing), and "A happens before what stream S is given next" is A's snapshot <= S's clock.  Every call is counted.  Built from the header
// alone (tests/test_cpp_order.py); prints one line per failed check and "ok" when there is none.
#include <array>
#include <cstdint>
#include <cstdio>

#include "../../ice_halo_sim_amd/csrc/halo_order.h"

using namespace halo;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      failures++;                                         \
      std::printf("line %d: %s: ", __LINE__, #cond);      \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
    }                                                     \
  } while (0)

struct Clock {
  std::array<uint64_t, 8> v{};
  void join(const Clock& o) {
    for (size_t i = 0; i < v.size(); i++) v[i] = v[i] > o.v[i] ? v[i] : o.v[i];
  }
  bool le(const Clock& o) const {
    for (size_t i = 0; i < v.size(); i++)
      if (v[i] > o.v[i]) return false;
    return true;
  }
};
struct FakeStream {
  int id = 0;
  Clock c;
};
struct FakeEvent {
  Clock c;
  bool recorded = false, timed = false;
};
struct Fake {
  using Stream = FakeStream*;
  using Event = FakeEvent*;
  using Error = int;
  static constexpr Error kOk = 0;
  static inline int records = 0, waits = 0, syncs = 0, timed_made = 0, untimed_made = 0, made = 0;
  static inline int live_streams = 0, live_events = 0, next_id = 0;
  static inline int fail_at = -1;          // the creation (streams and events counted together) that fails, -1: none
  static inline bool order_broken = false; // destroy: an event dropped before every stream was waited for, or a stream before every event
  static inline int syncs_owed = 0;
  static void reset() { records = waits = syncs = 0; }
  static int calls() { return records + waits + syncs; }
  static Error record(Event e, Stream s) {
    records++;
    e->c = s->c, e->recorded = true;
    return kOk;
  }
  static Error wait(Stream s, Event e) {
    waits++;
    if (e->recorded) s->c.join(e->c);
    return kOk;
  }
  static Error sync(Stream) {
    syncs++;
    if (syncs_owed > 0) syncs_owed--;
    return kOk;
  }
  static Error create_stream(Stream* s) {
    if (made++ == fail_at) return 1;
    *s = new FakeStream;
    (*s)->id = next_id++ % 8;
    live_streams++;
    return kOk;
  }
  static Error destroy_stream(Stream s) {
    if (live_events != 0) order_broken = true;
    delete s;
    live_streams--;
    return kOk;
  }
  static Error create_event(Event* e, bool timed) {
    if (made++ == fail_at) return 1;
    *e = new FakeEvent;
    (*e)->timed = timed;
    (timed ? timed_made : untimed_made)++;
    live_events++;
    return kOk;
  }
  static Error destroy_event(Event e) {
    if (syncs_owed != 0) order_broken = true;
    delete e;
    live_events--;
    return kOk;
  }
};
using Ord = StreamOrder<Fake>;

// Work queued on a stream: its snapshot.
static Clock work(FakeStream* s) {
  s->c.v[static_cast<size_t>(s->id)]++;
  return s->c;
}
// `a` happens before what stream `s` is given next.
static bool before(const Clock& a, const FakeStream* s) { return a.le(s->c); }

struct Rig {
  Options opt;
  Ord o{&opt};
  Rig(int overlap, int lean) {
    opt.overlap = overlap, opt.lean_events = lean;
    Fake::fail_at = -1, Fake::next_id = 0;   // (this handle's streams are components 0..3 of the clocks; a caller's stream takes 7)
    const int rc = o.create();
    CHECK(rc == Fake::kOk, "create failed");
    Fake::reset();
  }
  // a launch as queue_launch makes one: the stream choice, then a trace kernel on it
  Clock launch(bool touches_planes, bool alternate, FakeStream** ts, int* i) {
    const int rc = o.next_trace_stream(touches_planes, alternate, ts, i);
    CHECK(rc == Fake::kOk, "next_trace_stream failed");
    return work(*ts);
  }
};

static void ownership() {
  const int made0 = Fake::made;
  {
    Rig r(1, 1);
    CHECK(Fake::live_streams == 4 && Fake::live_events == 17 + 5 * Ord::kRing, "streams %d events %d", Fake::live_streams, Fake::live_events);
    CHECK(Fake::timed_made == 4 * Ord::kRing && Fake::untimed_made == 17 + Ord::kRing, "timed %d untimed %d", Fake::timed_made, Fake::untimed_made);
    CHECK(r.o.main == r.o.own && r.o.own != nullptr && r.o.ring[Ord::kRing - 1].ev0->timed && !r.o.ring[0].done->timed && !r.o.close_done.ev->timed, "handles");
    Fake::syncs_owed = 4;   // main, auxiliary, both trace streams: before the first event goes
    r.o.destroy();
    CHECK(Fake::syncs == 4 && Fake::live_streams == 0 && Fake::live_events == 0 && !Fake::order_broken, "destroy: syncs %d streams %d events %d", Fake::syncs, Fake::live_streams, Fake::live_events);
    Fake::reset();
    r.o.destroy();   // nothing left: nothing done
    CHECK(Fake::calls() == 0, "second destroy made %d calls", Fake::calls());
  }
  const int all = Fake::made - made0;
  // a caller's main stream is waited for and left alone
  {
    Rig r(1, 1);
    FakeStream other;
    other.id = 7;
    r.o.set_main(&other);
    Fake::reset();
    Fake::syncs_owed = 4;
    r.o.destroy();
    CHECK(Fake::syncs == 4 && Fake::live_streams == 0 && Fake::live_events == 0 && !Fake::order_broken, "destroy with a caller's stream");
  }
  // a partly created handle cleans up through the same path, whichever creation fails
  for (int at = 0; at < all; at++) {
    Options opt;
    Ord o(&opt);
    Fake::made = 0, Fake::fail_at = at;
    CHECK(o.create() != Fake::kOk, "creation %d should have failed", at);
    o.destroy();
    CHECK(Fake::live_streams == 0 && Fake::live_events == 0 && !Fake::order_broken, "failed creation %d leaves streams %d events %d", at, Fake::live_streams, Fake::live_events);
  }
  Fake::fail_at = -1;
}

// 1. Fork: what the auxiliary stream is given after fork_aux() is behind everything main and both pending trace streams held.
static void fork_scenario(int ov, int lean) {
  Rig r(ov, lean);
  const Clock m = work(r.o.main_q());
  FakeStream *t0 = nullptr, *t1 = nullptr;
  int i0 = 0, i1 = 0;
  const Clock k0 = r.launch(false, true, &t0, &i0), k1 = r.launch(false, true, &t1, &i1);
  const Clock m2 = work(r.o.main_q());
  Fake::reset();
  CHECK(r.o.fork_aux() == Fake::kOk, "fork_aux");
  FakeStream* ps = r.o.post_stream();
  if (!ov) CHECK(ps == r.o.main && Fake::calls() == 0, "overlap 0: post stream is main, fork makes %d calls", Fake::calls());
  else CHECK(ps == r.o.aux && Fake::records == 3 && Fake::waits == 3, "fork: %d records %d waits", Fake::records, Fake::waits);
  CHECK(before(m, ps) && before(m2, ps) && before(k0, ps) && before(k1, ps), "overlap %d lean %d: the post stream is not behind main and both trace streams", ov, lean);
}

// 2. Join: what main is given next is behind everything queued on the auxiliary and both trace streams; nothing new, no call; the markers it clears.
static void join_scenario(int ov, int lean) {
  Rig r(ov, lean);
  FakeStream *t0 = nullptr, *t1 = nullptr;
  int i0 = 0, i1 = 0;
  const Clock k0 = r.launch(false, true, &t0, &i0);
  CHECK(r.o.sums_queued(t0, i0, true) == Fake::kOk, "sums_queued");
  const Clock k1 = r.launch(false, true, &t1, &i1);
  CHECK(r.o.close_marks(r.o.ring[1], t1, i1, 0) == Fake::kOk, "close_marks");
  CHECK(r.o.fork_aux() == Fake::kOk, "fork_aux");
  const Clock f = work(r.o.post_stream());
  if (ov) CHECK(i0 == 0 && i1 == 1 && r.o.rmw[0].set && r.o.close_done.set && r.o.close_ts == 1, "setup");
  CHECK(r.o.join() == Fake::kOk, "join");
  CHECK(before(k0, r.o.main) && before(k1, r.o.main) && before(f, r.o.main), "overlap %d lean %d: main is not behind the auxiliary and the trace streams", ov, lean);
  Fake::reset();
  CHECK(r.o.join() == Fake::kOk && Fake::calls() == 0, "a second join made %d calls", Fake::calls());
  if (ov) {
    CHECK(!r.o.rmw[0].set && !r.o.close_done.set, "join left rmw / close_done set");
    CHECK(r.o.rmw[0].wait_on(t1) == Fake::kOk && r.o.close_done.wait_on(t0) == Fake::kOk && r.o.behind_other_close(t0, 0) == Fake::kOk && Fake::calls() == 0, "cleared markers made %d calls", Fake::calls());
  }
  CHECK(r.o.sync_all() == Fake::kOk && Fake::syncs == 1 && Fake::records == 0 && Fake::waits == 0, "sync_all with nothing pending: %d syncs", Fake::syncs);
}

// 3. Alternation.
static void alternation_scenario(int ov, int lean) {
  Rig r(ov, lean);
  FakeStream* ts = nullptr;
  int i = 0;
  for (int k = 0; k < 5; k++) {
    r.launch(false, true, &ts, &i);
    if (ov) CHECK(i == (k & 1) && ts == r.o.cs[k & 1], "alternate launch %d went to trace stream %d", k, i);
    else CHECK(i == 0 && ts == r.o.main, "overlap 0: launch %d", k);
  }
  for (int k = 0; k < 3; k++) {
    r.launch(false, false, &ts, &i);
    CHECK(i == 0 && ts == (ov ? r.o.cs[0] : r.o.main), "a launch that fills the chip went to trace stream %d", i);
  }
  if (!ov) CHECK(Fake::calls() == 0, "overlap 0: %d calls", Fake::calls());
}

// 4. The hop from the main stream.
static void hop_scenario(int ov, int lean) {
  Rig r(ov, lean);
  FakeStream* ts = nullptr;
  int i = 0;
  CHECK(r.o.main_dirty[0] && r.o.main_dirty[1], "a new handle's trace streams have seen nothing of main");
  Clock m = work(r.o.main_q());
  r.launch(false, false, &ts, &i);
  CHECK(before(m, ts), "overlap %d lean %d: the first launch is not behind main", ov, lean);
  if (!ov) return;
  Fake::reset();
  r.launch(false, false, &ts, &i);   // nothing new on main
  if (lean) CHECK(Fake::calls() == 0, "lean: a second launch with nothing new on main made %d calls", Fake::calls());
  else CHECK(Fake::records == 1 && Fake::waits == 1, "every launch hops: %d records %d waits", Fake::records, Fake::waits);
  m = work(r.o.main_q());
  Fake::reset();
  r.launch(false, false, &ts, &i);
  CHECK(Fake::records == 1 && Fake::waits == 1 && before(m, ts), "after main_q the launch hops again: %d records %d waits", Fake::records, Fake::waits);
  // a caller's stream may hold work the unit never saw: hopped every time
  FakeStream other;
  other.id = 7;
  r.o.main_dirty[0] = r.o.main_dirty[1] = false;
  r.o.set_main(&other);
  CHECK(r.o.main == &other && r.o.main_dirty[0] && r.o.main_dirty[1], "set_main marks both trace streams dirty");
  for (int k = 0; k < 3; k++) {
    m = work(&other);   // (not through main_q)
    Fake::reset();
    r.launch(false, false, &ts, &i);
    CHECK(Fake::records == 1 && Fake::waits == 1 && before(m, ts), "a caller's main stream, launch %d: %d records %d waits", k, Fake::records, Fake::waits);
  }
  r.o.main_dirty[0] = r.o.main_dirty[1] = false;
  r.o.set_main(nullptr);
  CHECK(r.o.main == r.o.own && r.o.main_dirty[0] && r.o.main_dirty[1], "back to the own stream: both trace streams dirty");
  for (int k = 0; k < 2; k++) {
    Fake::reset();
    r.launch(false, true, &ts, &i);
    CHECK(Fake::records == 1 && Fake::waits == 1, "after set_main trace stream %d hops", i);
  }
}

// 5. Behind the fold.
static void fold_scenario(int ov, int lean) {
  FakeStream* ts = nullptr;
  int i = 0;
  {
    Rig r(ov, lean);
    CHECK(r.o.fork_aux() == Fake::kOk, "fork_aux");
    const Clock f = work(r.o.post_stream());
    r.launch(true, false, &ts, &i);
    CHECK(before(f, ts), "overlap %d lean %d: a launch that touches the planes is not behind the fold", ov, lean);
  }
  if (!ov) return;
  Rig r(ov, lean);
  CHECK(r.o.fork_aux() == Fake::kOk, "fork_aux");
  Clock f = work(r.o.post_stream());
  Fake::reset();
  r.launch(false, false, &ts, &i);
  CHECK(Fake::records == 1 && Fake::waits == 1 && !before(f, ts), "under the fold: the hop alone, %d records %d waits", Fake::records, Fake::waits);
  Fake::reset();
  CHECK(r.o.wait_for_aux(i) == Fake::kOk && Fake::records == 1 && Fake::waits == 1 && before(f, ts), "wait_for_aux orders the trace stream");
  Fake::reset();
  CHECK(r.o.wait_for_aux(i) == Fake::kOk && Fake::calls() == 0, "a second wait_for_aux made %d calls", Fake::calls());
  CHECK(r.o.wait_for_aux(1) == Fake::kOk && Fake::records == 1 && Fake::waits == 1, "the other trace stream has not seen the fold");
  CHECK(r.o.fork_aux() == Fake::kOk, "fork_aux");
  f = work(r.o.post_stream());
  Fake::reset();
  CHECK(r.o.wait_for_aux(i) == Fake::kOk && Fake::records == 1 && Fake::waits == 1 && before(f, ts), "a new fork is waited for again");
  CHECK(r.o.join() == Fake::kOk, "join");
  Fake::reset();
  CHECK(r.o.wait_for_aux(1) == Fake::kOk && Fake::calls() == 0, "nothing pending on the auxiliary stream: %d calls", Fake::calls());
}

// 6. Markers.
static void marker_scenario(int ov, int lean) {
  Rig r(ov, lean);
  FakeStream *s1 = r.o.cs[0], *s2 = r.o.cs[1];
  Ord::Marker& m = r.o.set_free[1];
  CHECK(m.wait_on(s2) == Fake::kOk && Fake::calls() == 0, "wait_on before any mark made %d calls", Fake::calls());
  const Clock w0 = work(s1);
  CHECK(m.mark(s1) == Fake::kOk && Fake::records == 1 && m.at == m.ev, "mark");
  CHECK(m.wait_on(s2) == Fake::kOk && Fake::waits == 1 && before(w0, s2), "the waiter is behind the marked work");
  FakeEvent* shared = r.o.ring[3].ev3;
  work(s1);
  Fake::record(shared, s1);
  Fake::reset();
  CHECK(m.mark_at(shared) == Fake::kOk && Fake::calls() == 0 && m.at == shared && m.set, "mark_at records nothing");
  const Clock w2 = work(s1);
  Fake::record(shared, s1);   // the ring slot comes round before the marker is marked again
  CHECK(!before(w2, s2), "setup");
  CHECK(m.wait_on(s2) == Fake::kOk && before(w2, s2), "a shared event recorded again: the waiter is behind the later point");
  Fake::reset();
  m.clear();
  CHECK(Fake::calls() == 0 && m.wait_on(s2) == Fake::kOk && Fake::calls() == 0, "clear / wait_on after clear made %d calls", Fake::calls());
}

// 7. Plane ownership between the two trace streams.
static void planes_scenario(int ov, int lean) {
  FakeStream *ta = nullptr, *tb = nullptr, *tc = nullptr;
  int ia = 0, ib = 0, ic = 0;
  {   // rule 1, then rule 2
    Rig r(ov, lean);
    const Clock a = r.launch(false, true, &ta, &ia);
    r.launch(false, true, &tb, &ib);
    FakeEvent* gate = nullptr;
    Fake::reset();
    CHECK(r.o.gate_sums(ib, &gate) == Fake::kOk, "gate_sums");
    const Clock later = work(ta);   // queued on the other stream after the launch: not what the sums wait for
    if (!ov) {
      CHECK(gate == nullptr && Fake::calls() == 0 && r.o.sums_queued(tb, ib, true) == Fake::kOk && r.o.behind_other_sums(tb, ib) == Fake::kOk && Fake::calls() == 0, "overlap 0: %d calls", Fake::calls());
      return;
    }
    CHECK(ia == 0 && ib == 1 && gate != nullptr && Fake::records == 1 && Fake::waits == 0, "gate: %d records", Fake::records);
    Fake::wait(tb, gate);   // (the passes wait for it in front of their first plain write)
    const Clock sums = work(tb);
    CHECK(before(a, tb) && !before(later, tb), "the sums are behind what the other trace stream held when the launch was queued, and no more");
    CHECK(r.o.sums_queued(tb, ib, true) == Fake::kOk && r.o.rmw[ib].set, "the sums leave their marker");
    r.launch(false, true, &tc, &ic);
    CHECK(ic == 0 && !before(sums, tc), "setup");
    CHECK(r.o.behind_other_sums(tc, ic) == Fake::kOk && before(sums, tc), "a launch that adds to the planes itself is behind the other stream's sums");
  }
  {   // no gate while the other trace stream holds nothing; the integer route leaves no marker
    Rig r(ov, lean);
    r.launch(false, true, &ta, &ia);
    FakeEvent* gate = r.o.ev_gate;
    Fake::reset();
    CHECK(r.o.gate_sums(ia, &gate) == Fake::kOk && gate == nullptr && Fake::calls() == 0, "gate with the other stream idle: %d calls", Fake::calls());
    CHECK(r.o.sums_queued(ta, ia, false) == Fake::kOk && !r.o.rmw[ia].set && Fake::calls() == 0, "the integer route left an rmw marker");
    CHECK(r.o.behind_other_sums(r.o.cs[1], 1) == Fake::kOk && Fake::calls() == 0, "no sums, no wait");
  }
  {   // a direct close on the other trace stream
    Rig r(ov, lean);
    r.launch(false, true, &ta, &ia);
    const Clock c = work(ta);   // the closing pass
    CHECK(r.o.close_marks(r.o.ring[0], ta, ia, 0) == Fake::kOk && r.o.close_ts == ia, "close_marks");
    r.launch(false, true, &tb, &ib);
    CHECK(!before(c, tb), "setup");
    CHECK(r.o.behind_other_close(tb, ib) == Fake::kOk && before(c, tb), "a launch on the other stream is behind a direct close");
    r.launch(false, true, &tc, &ic);
    Fake::reset();
    CHECK(ic == ia && r.o.behind_other_close(tc, ic) == Fake::kOk && Fake::calls() == 0, "the close's own stream waits for nothing: %d calls", Fake::calls());
  }
}

// 8. The four markers behind a direct close.
static void close_scenario(int ov, int lean) {
  Rig r(ov, lean);
  FakeStream* ts = nullptr;
  int i = 0;
  r.launch(false, true, &ts, &i);
  Ord::RingSlot& slot = r.o.ring[5];
  Fake::reset();
  CHECK(r.o.passes_begin(slot, ts, true) == Fake::kOk, "passes_begin");
  if (lean) CHECK(Fake::records == 0 && slot.t2 == slot.ev1, "lean: ev1 carries the passes' begin");
  else CHECK(Fake::records == 1 && slot.t2 == slot.ev2, "ev2 recorded for the passes' begin");
  Fake::reset();
  CHECK(r.o.passes_begin(slot, ts, false) == Fake::kOk && Fake::records == 1 && slot.t2 == slot.ev2, "a wait lies between: ev2 is recorded");
  const Clock c = work(ts);   // the closing pass
  Fake::reset();
  CHECK(r.o.close_marks(slot, ts, i, 1) == Fake::kOk && Fake::waits == 0 && r.o.close_ts == i, "close_marks");
  if (lean) CHECK(Fake::records == 1 && r.o.close_done.set && r.o.close_done.at == slot.ev3 && r.o.set_free[1].set && r.o.set_free[1].at == slot.ev3 && slot.fin == slot.ev3, "lean: %d records", Fake::records);
  else CHECK(Fake::records == 4 && r.o.close_done.at == r.o.close_done.ev && r.o.set_free[1].at == r.o.set_free[1].ev && slot.fin == slot.done, "four records: %d", Fake::records);
  CHECK(slot.ev3->recorded && slot.fin->recorded && slot.fin->c.le(ts->c) && c.le(slot.fin->c), "the slot's last event is behind the closing pass");
  CHECK(r.o.set_free[1].wait_on(r.o.main_q()) == Fake::kOk && before(c, r.o.main), "overlap %d lean %d: the log set's next user is not behind the closing pass", ov, lean);
  Fake::reset();
  CHECK(r.o.slot_done(slot, ts) == Fake::kOk && Fake::records == 1 && slot.fin == slot.done, "slot_done");
}

// 9. The dispatch ring.
static void ring_scenario(int ov, int lean) {
  Rig r(ov, lean);
  bool harvest = true;
  for (int k = 0; k < Ord::kRing; k++) {
    const int got = r.o.take(&harvest);
    CHECK(got == k && !harvest && r.o.ring[k].use == 1, "first round: slot %d, harvest %d", got, int(harvest));
    r.o.ring[k].busy = (k % 3) != 0;   // (queue_launch sets it; harvest_slot clears it)
  }
  const uint64_t use7 = r.o.ring[7].use;
  CHECK(r.o.reader_alive(7, use7) && !r.o.reader_alive(6, r.o.ring[6].use) && !r.o.reader_alive(7, use7 - 1), "reader_alive");
  Fake::record(r.o.ring[7].done, r.o.cs[0]);
  r.o.ring[7].fin = r.o.ring[7].done;
  r.o.main_dirty[0] = r.o.main_dirty[1] = false;
  Fake::reset();
  CHECK(r.o.behind_reader(6, r.o.ring[6].use) == Fake::kOk && Fake::calls() == 0 && !r.o.main_dirty[0], "a harvested reader: no wait");
  CHECK(r.o.behind_reader(7, use7) == Fake::kOk && Fake::waits == 1 && Fake::records == 0 && r.o.main_dirty[0] && r.o.main_dirty[1], "a live reader: main waits, through main_q");
  for (int k = 0; k < Ord::kRing; k++) {
    const int got = r.o.take(&harvest);
    CHECK(got == k && harvest == ((k % 3) != 0) && r.o.ring[k].use == 2, "the ring wraps: slot %d, harvest %d", got, int(harvest));
    r.o.ring[k].busy = false;   // harvested
  }
  r.o.ring[7].busy = true;   // the slot's NEXT launch is in flight
  CHECK(!r.o.reader_alive(7, use7), "reader_alive after the slot has been taken again");
  r.o.take(&harvest);
  CHECK(!harvest, "a harvested slot is not reported again");
}

int main() {
  ownership();
  for (int ov = 0; ov < 2; ov++)
    for (int lean = 0; lean < 2; lean++) {
      fork_scenario(ov, lean);
      join_scenario(ov, lean);
      alternation_scenario(ov, lean);
      hop_scenario(ov, lean);
      fold_scenario(ov, lean);
      marker_scenario(ov, lean);
      planes_scenario(ov, lean);
      close_scenario(ov, lean);
      ring_scenario(ov, lean);
    }
  CHECK(Fake::live_streams == 0 && Fake::live_events == 0 && !Fake::order_broken, "left behind: streams %d events %d", Fake::live_streams, Fake::live_events);
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
