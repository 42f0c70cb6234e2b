// halo_order.h — the stream order of a handle as one unit: the four streams, every event that orders them, the markers, the plane-ownership rules
// between the two trace streams and the dispatch ring — which stream waits for which event, and when a wait may be left out.  Standard library
// only, no HIP: the calls come from an API type (halo_state.h gives the real ones, HipOrderApi), and tests/cpp/order_main.cpp compiles this header
// alone against a vector-clock model of streams and events and checks every rule as a happens-before statement on the CPU.
//
// The API type provides: Stream, Event and Error (with kOk), record(event, stream), wait(stream, event), sync(stream), create_stream / destroy_stream,
// create_event(event*, timed) / destroy_event.  A default-constructed handle is "none".
#ifndef HALO_ORDER_H_
#define HALO_ORDER_H_

#include <cstdint>
#include <vector>

#include "halo_options.h"

namespace halo {

#define HALO_ORDER_TRY(call)            \
  do {                                  \
    const Error e__ = (call);           \
    if (e__ != Api::kOk) return e__;    \
  } while (0)

template <class Api>
struct StreamOrder {
  using Stream = typename Api::Stream;
  using Event = typename Api::Event;
  using Error = typename Api::Error;

  // "The last work of kind X": an event recorded behind that work, and whether anything has been recorded on it yet (nothing: nobody need wait).
  // (Several markers that fall on one point of one stream share one recorded event: mark_at names an event somebody has just recorded there — a ring
  //  slot's — instead of recording the marker's own.  Should that event be recorded again before the marker is, the marker waits for the later point.)
  struct Marker {
    Event ev{};
    Event at{};   // the event that carries the marker now: `ev`, or a shared one
    bool set = false;
    Error mark(Stream s) {
      const Error e = Api::record(ev, s);
      if (e == Api::kOk) at = ev, set = true;
      return e;
    }
    Error mark_at(Event shared) {
      at = shared, set = true;
      return Api::kOk;
    }
    Error wait_on(Stream s) const { return set ? Api::wait(s, at) : Api::kOk; }
    void clear() { set = false; }
  };

  // One slot of the dispatch ring: the events of the launch that holds it and what harvest_slot (halo_backend.cpp) needs to take its timing.
  struct RingSlot {
    Event ev0{}, ev1{}, ev2{}, ev3{}, done{};   // ev0..ev1 the trace kernel (trace stream), ev2..ev3 its passes (post stream); done is untimed
    // (the events that CARRY the slot's "passes begin" and "slot done" for its current launch: ev2 / done themselves, or — option lean_events —
    //  the neighbour recorded at the same point of the same stream: ev1 where no wait lies between it and the passes, ev3 behind a direct close)
    Event t2{}, fin{};
    bool posts = false;
    bool final = false;   // the slot's launch belongs to its session's last layer (halo_collect_timing counts those)
    bool busy = false;
    uint64_t use = 0;     // how many launches have taken the slot (TableCacheEntry::read_use)
  };
  static constexpr int kRing = 32;

  const Options* opt;   // the two bits read here: overlap, lean_events
  Stream own{};         // the handle's own main stream
  Stream main{};        // the main stream in use: `own`, or the caller's (set_main)
  // Auxiliary stream (round 5): the closing folds are queued here, behind everything the other streams hold, and nobody waits for them until
  // somebody reads the image or adds to the planes again — a session's fold (20 us) runs under the next session's first kernels instead of
  // in front of them.  (Two engines side by side on one GPU had measured +10 .. 15 % over one, tools/two_engines_probe.py; what that was,
  // looked at inside one engine, is the small things between kernels — folds, resets, uploads, the tails — not the trace kernels or their
  // passes, which gain nothing from running under each other: see queue_passes.)
  Stream aux{};
  Event ev_fork{}, ev_join{};
  bool aux_pending = false;   // work has been queued on `aux` that the main stream has not waited for
  // Two trace streams: consecutive launches alternate between them, so that launch k+1's workgroups fill the CUs that launch k's last
  // workgroups leave idle (kernels of ONE stream run one after the other: the tail of every 1.8 ms trace kernel, and the whole of a
  // latency-bound small launch, went unshared).  Trace kernels of different launches have nothing to order between them: each logs to its own
  // buffer set or adds with atomics, tallies and continuation appends are atomic.  What they must follow is on the main stream (table
  // uploads) or the auxiliary one (a fold or per-tile pass before a launch that adds to the planes itself): waited for by events.
  Stream cs[2] = {};
  Event ev_cs[2] = {}, ev_main{}, ev_aux{};
  bool cs_pending[2] = {false, false};
  int cs_next = 0;
  bool main_dirty[2] = {true, true};   // the main stream has been given work (main_q) since trace stream i last waited for it
  uint64_t aux_seq = 0, cs_seen_aux[2] = {0, 0};   // (a trace stream waits for the auxiliary stream only when that holds work it has not waited for yet)
  Event ev_gen{};   // the generator of a chip-filling launch, queued on trace stream 1 (option gen_ahead)

  Marker set_free[2];      // the passes that last read log set s (they may still be running)
  Marker set_folded[2];    // the fold that last zeroed plane set s
  Marker shapes_free[2];   // the trace kernel that last read shape pool s
  // Plane ownership between the two trace streams.  The per-tile sums of a logged (or two-level binned) launch end in PLAIN read-modify-writes of
  // the planes; everything else that adds to them uses atomics.  So (1) a launch's sums wait for what the OTHER trace stream held when the launch
  // was queued (ev_gate), and (2) a later launch on the other stream whose trace kernel adds to the planes itself waits for those sums (rmw).
  // Logged trace kernels touch no plane (their overflow goes to the fp64 twin), so they run beside a neighbour's passes freely.
  Event ev_gate{};
  Marker rmw[2];           // the per-tile sums last queued on trace stream i
  // A direct close is a PLAIN read-modify-write of the image and of the twin's half, on the launch's trace stream: a later launch on
  // the other trace stream waits for it, readers and folds join the trace streams as they always do.
  Marker close_done;       // the direct close queued last, on trace stream close_ts
  int close_ts = 0;

  RingSlot ring[kRing];
  int ring_next = 0;

  explicit StreamOrder(const Options* o) : opt(o) {}
  StreamOrder(const StreamOrder&) = delete;
  StreamOrder& operator=(const StreamOrder&) = delete;
  ~StreamOrder() { destroy(); }

  // ---- ownership ----
  // The main stream first (a handle without one is no handle), then the other streams, the untimed events and the ring's.  Whatever exists when a
  // step fails is dropped by destroy().
  Error create() {
    HALO_ORDER_TRY(new_stream(&own));
    main = own;
    HALO_ORDER_TRY(new_stream(&aux));
    HALO_ORDER_TRY(new_stream(&cs[0]));
    HALO_ORDER_TRY(new_stream(&cs[1]));
    for (Event* e : {&ev_cs[0], &ev_cs[1], &ev_main, &ev_aux, &ev_fork, &ev_join, &ev_gen, &ev_gate, &set_free[0].ev, &set_free[1].ev, &shapes_free[0].ev,
                     &shapes_free[1].ev, &rmw[0].ev, &rmw[1].ev, &set_folded[0].ev, &set_folded[1].ev, &close_done.ev})
      HALO_ORDER_TRY(new_event(e, false));
    for (RingSlot& r : ring) {
      for (Event* e : {&r.ev0, &r.ev1, &r.ev2, &r.ev3}) HALO_ORDER_TRY(new_event(e, true));
      HALO_ORDER_TRY(new_event(&r.done, false));
    }
    return Api::kOk;
  }
  // Host waits for every stream, then the events go, then the streams (the caller's main stream is waited for and left alone).
  void destroy() {
    if (main != Stream{}) (void)Api::sync(main);
    for (Stream s : {aux, cs[0], cs[1]})
      if (s != Stream{}) (void)Api::sync(s);
    for (Event e : events_) (void)Api::destroy_event(e);
    for (Stream s : streams_) (void)Api::destroy_stream(s);
    events_.clear();
    streams_.clear();
    own = main = aux = cs[0] = cs[1] = Stream{};
  }

  // ---- the streams ----
  // The main stream, for whoever queues work on it (or waits for it): the trace streams have not seen that work yet (next_trace_stream).
  Stream main_q() {
    main_dirty[0] = main_dirty[1] = true;
    return main;
  }
  // Another main stream (none: the handle's own again), once everything queued so far is over: the trace streams have seen nothing of it.
  void set_main(Stream s) {
    (void)sync_all();
    main = s != Stream{} ? s : own;
    main_dirty[0] = main_dirty[1] = true;
  }
  // What the main stream is given from here on runs behind everything queued on the auxiliary and the trace streams (no host wait).
  Error join() {
    if (aux_pending) {
      HALO_ORDER_TRY(Api::record(ev_join, aux));
      HALO_ORDER_TRY(Api::wait(main_q(), ev_join));   // (main_q: the trace streams reach this wait through their next hop)
      aux_pending = false;
    }
    for (int k = 0; k < 2; k++)
      if (cs_pending[k]) {
        HALO_ORDER_TRY(Api::record(ev_cs[k], cs[k]));
        HALO_ORDER_TRY(Api::wait(main_q(), ev_cs[k]));
        cs_pending[k] = false;
        rmw[k].clear();   // (every later launch waits for the main stream, which now waits for these sums)
        if (close_ts == k) close_done.clear();   // ... and for this direct close
      }
    return Api::kOk;
  }
  // Host waits for all streams.
  Error sync_all() {
    HALO_ORDER_TRY(join());
    return Api::sync(main_q());
  }
  // The stream the plane-touching passes of logged launches and the folds are queued on.
  Stream post_stream() const { return opt->overlap ? aux : main; }
  // What is queued on the auxiliary stream from here on runs behind everything the main stream and the trace streams hold now.
  Error fork_aux() {
    if (!opt->overlap) return Api::kOk;
    HALO_ORDER_TRY(Api::record(ev_fork, main_q()));
    HALO_ORDER_TRY(Api::wait(aux, ev_fork));
    for (int k = 0; k < 2; k++)
      if (cs_pending[k]) {
        HALO_ORDER_TRY(Api::record(ev_cs[k], cs[k]));
        HALO_ORDER_TRY(Api::wait(aux, ev_cs[k]));
      }
    aux_pending = true;
    aux_seq++;
    return Api::kOk;
  }
  // Trace stream i goes on behind what the auxiliary stream holds now (a closing fold: it reads and zeroes the planes).
  Error wait_for_aux(int i) {
    if (opt->overlap && aux_pending && cs_seen_aux[i] != aux_seq) {
      HALO_ORDER_TRY(Api::record(ev_aux, aux));
      HALO_ORDER_TRY(Api::wait(cs[i], ev_aux));
      cs_seen_aux[i] = aux_seq;
    }
    return Api::kOk;
  }
  // The stream the next trace kernel goes to: behind what the main stream holds now (table uploads, counter resets) and — for a launch that
  // adds to the planes itself — behind what the auxiliary stream holds (folds, per-tile passes).
  Error next_trace_stream(bool touches_planes, bool alternate, Stream* out, int* which) {
    if (!opt->overlap) {
      *out = main;
      *which = 0;
      return Api::kOk;
    }
    // Launches alternate streams only while they are latency-bound (up to 2^21 rays: tools/dispatch_probe.cpp, us per session with / without,
    // 2^16 18.8 / 30.6, 2^18 25.2 / 44.0, 2^20 65.5 / 110, 2^22 264 / 250, 2^24 817 / 820); a launch that fills the chip by itself gains nothing
    // from a neighbour and keeps stream 0, where its HIP events time it undisturbed.
    const int i = alternate ? cs_next : 0;
    if (alternate) cs_next ^= 1;
    // (the hop is for what the main stream has been given since this trace stream last waited for it — table uploads, counter resets: main_q.  With
    //  nothing new there it orders nothing, and option lean_events leaves it out.  A caller's stream may hold work this backend never saw: always hopped.)
    if (!opt->lean_events || main_dirty[i] || main != own) {
      HALO_ORDER_TRY(Api::record(ev_main, main));
      HALO_ORDER_TRY(Api::wait(cs[i], ev_main));
      main_dirty[i] = false;
    }
    if (touches_planes) HALO_ORDER_TRY(wait_for_aux(i));
    cs_pending[i] = true;
    *out = cs[i];
    *which = i;
    return Api::kOk;
  }
  // Option gen_ahead: the generator of a chip-filling launch goes to trace stream 1, and the launch's trace stream `ts` goes on behind it.
  Stream gen_ahead_stream() const { return cs[1]; }
  Error behind_generator(Stream ts) {
    HALO_ORDER_TRY(Api::record(ev_gen, cs[1]));
    HALO_ORDER_TRY(Api::wait(ts, ev_gen));
    cs_pending[1] = true;
    return Api::kOk;
  }

  // ---- plane ownership: a launch on trace stream ts (index ts_i) against the other one ----
  // A direct close on the other trace stream: it writes the image and the twin's half plainly.
  Error behind_other_close(Stream ts, int ts_i) const { return close_done.set && close_ts != ts_i ? close_done.wait_on(ts) : Api::kOk; }
  // Rule (2): this trace kernel adds to the planes itself: behind the other trace stream's sums.
  Error behind_other_sums(Stream ts, int ts_i) const { return opt->overlap ? rmw[ts_i ^ 1].wait_on(ts) : Api::kOk; }
  // Rule (1): these sums write plainly: behind what the other trace stream held when the launch was queued — the event they wait for in front of
  // their first plain write, or none when that stream holds nothing.
  Error gate_sums(int ts_i, Event* before_sums) {
    *before_sums = Event{};
    if (opt->overlap && cs_pending[ts_i ^ 1]) {
      HALO_ORDER_TRY(Api::record(ev_gate, cs[ts_i ^ 1]));
      *before_sums = ev_gate;
    }
    return Api::kOk;
  }
  // ... and such sums have been queued on stream `s` for trace stream ts_i (`plain` false — the integer routes, whose every add is atomic — leaves no marker).
  Error sums_queued(Stream s, int ts_i, bool plain) { return opt->overlap && plain ? rmw[ts_i].mark(s) : Api::kOk; }

  // ---- the dispatch ring ----
  // The next slot, for a launch.  *harvest: the ring has wrapped onto a launch nobody has harvested yet (the caller takes its timing first, which
  // blocks only if that launch is still in flight).
  int take(bool* harvest) {
    const int k = ring_next;
    ring_next = (k + 1) % kRing;
    *harvest = ring[k].busy;
    ring[k].use++;
    return k;
  }
  // The launch that took ring slot `slot` as its use number `use` has not been harvested: it may still be running.
  bool reader_alive(int slot, uint64_t use) const { return ring[slot].busy && ring[slot].use == use; }
  // The main stream goes on behind that launch while it is alive (the table cache's guard: no host wait).
  Error behind_reader(int slot, uint64_t use) { return reader_alive(slot, use) ? Api::wait(main_q(), ring[slot].fin) : Api::kOk; }
  // The passes of the slot's launch begin on `ps`.  (shared: nothing lies between ev1 and here, so under lean_events one record serves as both —
  // the spans stay the trace kernel's and the passes'.)
  Error passes_begin(RingSlot& r, Stream ps, bool shared) {
    if (opt->lean_events && shared) r.t2 = r.ev1;
    else {
      HALO_ORDER_TRY(Api::record(r.ev2, ps));
      r.t2 = r.ev2;
    }
    return Api::kOk;
  }
  // The slot's launch ends here on stream `s`.
  Error slot_done(RingSlot& r, Stream s) {
    HALO_ORDER_TRY(Api::record(r.done, s));
    r.fin = r.done;
    return Api::kOk;
  }
  // Behind a direct close four markers fall on one point of the stream — the close, the end of the passes' span, log set `ls` free again, the slot
  // done: one record, ev3, and the others name it (lean_events; otherwise each its own).
  Error close_marks(RingSlot& r, Stream ps, int ts_i, int ls) {
    HALO_ORDER_TRY(Api::record(r.ev3, ps));
    close_ts = ts_i;
    if (opt->lean_events) {
      (void)close_done.mark_at(r.ev3);
      (void)set_free[ls].mark_at(r.ev3);
      r.fin = r.ev3;
      return Api::kOk;
    }
    HALO_ORDER_TRY(close_done.mark(ps));
    HALO_ORDER_TRY(set_free[ls].mark(ps));
    return slot_done(r, ps);
  }

 private:
  std::vector<Stream> streams_;   // what create() made, in its order: all of it and nothing else goes in destroy()
  std::vector<Event> events_;
  Error new_stream(Stream* s) {
    HALO_ORDER_TRY(Api::create_stream(s));
    streams_.push_back(*s);
    return Api::kOk;
  }
  Error new_event(Event* e, bool timed) {
    HALO_ORDER_TRY(Api::create_event(e, timed));
    events_.push_back(*e);
    return Api::kOk;
  }
};

#undef HALO_ORDER_TRY

}  // namespace halo

#endif
