// m3t_ingest_plan.h -- the bookkeeping that orders asynchronous frame uploads (copy streams) and the launches that read
// the frames (compute stream) against each other; DESIGN.md section 1 ("Frame ingest") states the protocol.  Every
// function returns a decision that its caller (Ingest in m3t_hip_api.hip) carries out with runtime calls.
// Plain C++17, no HIP header: tests/cpp/ingest_plan_check.cpp checks it.
#pragma once

namespace m3t_ingest {

constexpr int kStepEvents = 16;  // step s records event s % kStepEvents
constexpr int kCopyStreams = 4;  // cameras are spread round-robin: per-copy DMA latencies overlap

struct Wait {  // for nothing, for step event `event`, or for everything the compute stream holds
  enum Kind { kNothing, kStepEvent, kComputeStream } kind;
  int event;
};
struct ReadMark {
  long step;  // what to stamp into last_read_step of the slots the launches read
  int event;  // the step event to record behind them (-1: none, and nothing to stamp)
};

struct Ledger {
  long step_counter = 0;  // launches marked as readers so far: the id of the next ones
  long copy_waited_step[kCopyStreams] = {-1, -1, -1, -1};  // the latest step each copy stream has waited for
  unsigned pending = 0;    // bit s: copy stream s has frames not yet ordered before the compute stream
  bool async = false;      // asynchronous ingest has started: readers are counted and record step events
  bool untracked = false;  // the compute stream holds launches that may read frames and are behind no step event

  // The first asynchronous upload (whatever ran before was not tracked by step events): true when the streams and
  // events still have to be created.
  bool Start() {
    if (async) return false;
    return async = untracked = true;
  }
  // Launches that may read frames and record no step event of their own (the sub-step calls, set_features).
  void LaunchedUntracked() { untracked |= async; }
  // What copy stream cs waits for before it overwrites a slot last read by step last_read (-1: none).  Untracked
  // launches: the host synchronises the compute stream, once -- that covers every step so far, too.  Otherwise the
  // reader's event, unless the stream has already waited for that step or a later one (a copy stream is in order: one
  // wait per step covers all of its cameras).  The event is taken by its index WITHOUT asking whether a later step has
  // recorded it again since: a recycled event is a later step of the same stream, and waits for the reader as well.
  Wait OrderCopy(int cs, long last_read) {
    if (untracked) {
      untracked = false;
      return {Wait::kComputeStream, -1};
    }
    if (last_read <= copy_waited_step[cs]) return {Wait::kNothing, -1};
    copy_waited_step[cs] = last_read;
    return {Wait::kStepEvent, int(last_read % kStepEvents)};
  }
  void CopyEnqueued(int cs) { pending |= 1u << cs; }
  // the copy streams the compute stream has to wait for before its next launches; none are pending afterwards
  unsigned TakePending() {
    const unsigned mask = pending;
    pending = 0;
    return mask;
  }
  // Launches that read frames have been enqueued (a tracking step, an enqueued call with cameras): they take a step id
  // and an event, and it is the next ones' turn.  Before the first asynchronous upload: nothing, the counter stays.
  ReadMark MarkRead() {
    if (!async) return {-1, -1};
    ++step_counter;
    return {step_counter - 1, int((step_counter - 1) % kStepEvents)};
  }
  // What the host waits for to see the last reader of a slot finished (camera_slot_sync of a rectangle slot).  Unlike
  // OrderCopy this side DOES ask whether the event is still the reader's: while last_read + kStepEvents > step_counter
  // it is, and the host waits for it alone; after that, for everything the compute stream holds.  Both rules are
  // conservative; they differ, and are kept as they are.
  Wait WaitForReader(long last_read) const {
    if (last_read < 0) return {Wait::kNothing, -1};
    if (last_read + kStepEvents > step_counter) return {Wait::kStepEvent, int(last_read % kStepEvents)};
    return {Wait::kComputeStream, -1};
  }
};

}  // namespace m3t_ingest
