// The ordering ledger of asynchronous frame ingest (3dobjecttracking_amd/csrc/m3t_ingest_plan.h) on the host: the ledger
// is run through written-down sequences of uploads and steps the way the library's entry points drive it, and every
// decision it returns is compared with what the protocol says must happen at that point -- typed
// in here, step ids counted from 0, 16 step events, 4 copy streams, camera c on copy stream c % 4.
// Prints "checks N errors M".
#include <cstdio>
#include <vector>

#include "../../3dobjecttracking_amd/csrc/m3t_ingest_plan.h"

using namespace m3t_ingest;

static int g_checks = 0, g_errors = 0;
#define CHECK(cond)                                  \
  do {                                               \
    ++g_checks;                                      \
    if (!(cond)) {                                   \
      ++g_errors;                                    \
      std::printf("line %d: %s\n", __LINE__, #cond); \
    }                                                \
  } while (0)

static bool Is(const Wait& w, Wait::Kind kind, int event = -1) { return w.kind == kind && w.event == event; }
static bool Is(const ReadMark& m, long step, int event) { return m.step == step && m.event == event; }

// cameras with rings of n_slots, driven as the library does it: an upload asks for its order and marks its copy stream,
// a step joins the pending copies and stamps the slots it reads
struct Rings {
  Ledger ledger;
  std::vector<std::vector<long>> last_read;  // [camera][slot]
  Rings(int n_cameras, int n_slots) : last_read(size_t(n_cameras), std::vector<long>(size_t(n_slots), -1)) {}
  Wait Upload(int camera, int slot) {
    const int cs = camera % 4;
    const Wait order = ledger.OrderCopy(cs, last_read[size_t(camera)][size_t(slot)]);
    ledger.CopyEnqueued(cs);
    return order;
  }
  ReadMark Step(int slot) {  // every camera's current slot
    const ReadMark mark = ledger.MarkRead();
    for (auto& camera : last_read) camera[size_t(slot)] = mark.step;
    return mark;
  }
};

// sub-step launches, then the first asynchronous upload: ONE synchronisation of the compute stream
static void FirstUpload() {
  Ledger l;
  l.LaunchedUntracked();  // before asynchronous ingest nothing is kept
  CHECK(!l.async && !l.untracked);
  CHECK(Is(l.MarkRead(), -1, -1) && l.step_counter == 0);  // ... and a step records no event
  CHECK(l.Start());  // streams and events are to be made
  CHECK(l.async && l.untracked);
  CHECK(Is(l.OrderCopy(0, -1), Wait::kComputeStream));
  CHECK(!l.untracked);
  CHECK(Is(l.OrderCopy(1, -1), Wait::kNothing));
  CHECK(Is(l.OrderCopy(0, -1), Wait::kNothing));
  CHECK(!l.Start());  // the second upload: nothing to make, nothing reset
  CHECK(l.async && !l.untracked);
  // a sub-step call later on: once again, and before any event wait (the slot was read by step 0)
  CHECK(Is(l.MarkRead(), 0, 0));
  l.LaunchedUntracked();
  CHECK(l.untracked);
  CHECK(Is(l.OrderCopy(2, 0), Wait::kComputeStream));
  CHECK(l.copy_waited_step[2] == -1);  // (the synchronisation is not remembered as a wait)
  CHECK(Is(l.OrderCopy(2, 0), Wait::kStepEvent, 0));
  CHECK(Is(l.OrderCopy(2, 0), Wait::kNothing));
}

// test_async_ingest_matches_blocking_upload for 40 steps: rings of two slots, frame s + 1 goes up behind step s into
// the slot step s - 1 read.  6 cameras: copy streams 0 and 1 carry two cameras each.
static void DoubleBuffer() {
  Rings r(6, 2);
  CHECK(r.ledger.Start());
  for (int c = 0; c < 6; ++c)  // the first frame, into slot 1: StartModalities ran before
    CHECK(Is(r.Upload(c, 1), c == 0 ? Wait::kComputeStream : Wait::kNothing));
  const int event_of_wait[40] = {-1, 0,  1,  2,  3,  4,  5,  6,  7, 8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2,
                                 3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6};
  for (int s = 0; s < 40; ++s) {
    CHECK(r.ledger.TakePending() == 0xFu);  // the step waits for all four copy streams, once
    CHECK(r.ledger.TakePending() == 0u);
    CHECK(Is(r.Step((s + 1) % 2), s, s % 16));
    CHECK(r.ledger.step_counter == s + 1);
    for (int c = 0; c < 6; ++c) {
      const Wait order = r.Upload(c, s % 2);
      if (s == 0)  // slot 0 was never read
        CHECK(Is(order, Wait::kNothing));
      else if (c < 4)  // the first camera of each copy stream: the event of step s - 1
        CHECK(Is(order, Wait::kStepEvent, event_of_wait[s]) && event_of_wait[s] == (s - 1) % 16);
      else  // cameras 4 and 5 share streams 0 and 1: already waited
        CHECK(Is(order, Wait::kNothing));
    }
    CHECK(r.ledger.copy_waited_step[0] == s - 1 && r.ledger.copy_waited_step[3] == s - 1);
  }
}

// rings of three slots: slot 2 is read by step 1 only, steps 2 .. 18 alternate between slots 0 and 1, then slot 2 is
// overwritten: event 1 is step 17's by now
static void RecycledEvent() {
  Rings r(2, 3);
  CHECK(r.ledger.Start());
  CHECK(Is(r.Upload(0, 0), Wait::kComputeStream));
  CHECK(Is(r.Step(0), 0, 0));
  CHECK(Is(r.Step(2), 1, 1));
  for (int s = 2; s <= 18; ++s) {
    CHECK(Is(r.Step(s % 2), s, s % 16));
    // camera 0 keeps uploading on copy stream 0, camera 1 (copy stream 1) is fed some other way
    const Wait order = r.Upload(0, (s + 1) % 2);
    if (s == 2)  // slot 1 has not been read yet
      CHECK(Is(order, Wait::kNothing));
    else
      CHECK(Is(order, Wait::kStepEvent, (s - 1) % 16));
  }
  CHECK(r.ledger.step_counter == 19 && r.last_read[0][2] == 1 && r.last_read[1][2] == 1);
  // the upload side takes the index of the reader's event, recycled or not: copy stream 1 has waited for nothing yet
  CHECK(Is(r.Upload(1, 2), Wait::kStepEvent, 1));
  CHECK(r.ledger.copy_waited_step[1] == 1);
  // ... and copy stream 0 has waited for step 17 already, which is behind step 1
  CHECK(r.ledger.copy_waited_step[0] == 17);
  CHECK(Is(r.Upload(0, 2), Wait::kNothing));
  // the slot-sync side: 19 steps so far, step 1 + 16 is not beyond them, so the whole compute stream
  CHECK(Is(r.ledger.WaitForReader(1), Wait::kComputeStream));
  CHECK(Is(r.ledger.WaitForReader(2), Wait::kComputeStream));
  CHECK(Is(r.ledger.WaitForReader(3), Wait::kComputeStream));  // (index 3 is the NEXT step's: given up one step early)
  CHECK(Is(r.ledger.WaitForReader(4), Wait::kStepEvent, 4));
  CHECK(Is(r.ledger.WaitForReader(17), Wait::kStepEvent, 1));
  CHECK(Is(r.ledger.WaitForReader(18), Wait::kStepEvent, 2));
  CHECK(Is(r.Step(2), 19, 3));  // step 19 reads slot 2; the decisions above changed nothing about the counter
  CHECK(Is(r.ledger.WaitForReader(4), Wait::kComputeStream));
  CHECK(Is(r.ledger.WaitForReader(5), Wait::kStepEvent, 5));
  CHECK(Is(r.ledger.WaitForReader(19), Wait::kStepEvent, 3));
}

// a slot that no step has read
static void NeverRead() {
  Rings r(1, 2);
  CHECK(r.ledger.Start());
  CHECK(Is(r.Upload(0, 0), Wait::kComputeStream));
  CHECK(Is(r.Step(0), 0, 0));
  CHECK(Is(r.Upload(0, 1), Wait::kNothing));
  CHECK(r.ledger.copy_waited_step[0] == -1);
  CHECK(Is(r.ledger.WaitForReader(-1), Wait::kNothing));
  CHECK(Is(r.ledger.WaitForReader(r.last_read[0][1]), Wait::kNothing));
  CHECK(Is(r.ledger.WaitForReader(r.last_read[0][0]), Wait::kStepEvent, 0));
}

// enqueued calls: reset_bodies reads the frames of its bodies' cameras and is marked like a step; judge_bodies without
// reset reads none, and the library asks nothing of the ledger for it
static void EnqueuedCalls() {
  Ledger l;
  CHECK(l.Start());
  CHECK(Is(l.OrderCopy(0, -1), Wait::kComputeStream));
  CHECK(Is(l.MarkRead(), 0, 0));  // a step
  CHECK(Is(l.MarkRead(), 1, 1));  // a call with cameras takes a step id of its own
  CHECK(l.step_counter == 2);
  CHECK(Is(l.MarkRead(), 2, 2));  // (a call without cameras in between: no mark, so) the next step follows at once
  CHECK(!l.untracked);  // none of them left the compute stream untracked
  CHECK(Is(l.OrderCopy(0, 1), Wait::kStepEvent, 1));  // a slot the call read waits for the call
}

static void PendingMask() {
  Ledger l;
  CHECK(l.TakePending() == 0u);
  l.CopyEnqueued(1);
  l.CopyEnqueued(3);
  l.CopyEnqueued(1);
  CHECK(l.pending == 0xAu);
  CHECK(l.TakePending() == 0xAu);
  CHECK(l.pending == 0u);
  CHECK(l.TakePending() == 0u);
}

int main() {
  static_assert(kStepEvents == 16 && kCopyStreams == 4, "the expectations below are written for these");
  FirstUpload();
  DoubleBuffer();
  RecycledEvent();
  NeverRead();
  EnqueuedCalls();
  PendingMask();
  std::printf("checks %d errors %d\n", g_checks, g_errors);
  return g_errors ? 1 : 0;
}
