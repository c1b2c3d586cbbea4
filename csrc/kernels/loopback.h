// Host side of the test-only loopback link (loopback.hip, parallel/loopback_comm.py).
//
// The link's control block is a /dev/shm file both processes map.  The GPU does not touch those pages:
// each process gives its kernels a page-locked control block of its own (hipHostMalloc, coherent), and a
// relay thread keeps the two in step word by word.  Every word has one writer, so the relay only copies:
// `out` words (written by this process's kernels) from the page-locked block to the shared one, `in` words
// (written by the peer's relay, or by either host for the abort word) the other way.
//
// What this costs and what it leaves out:
// * The thread polls about every 20 us plus the scheduler's slack, and a hand-off crosses two relays, so a
//   hop takes on the order of 100 us longer than through a block the GPU maps directly (from the code, not
//   measured).  The link is test-only; its throughput is set by the ring depth, not by this latency.
// * The thread ends with the pass that carries the abort word in.  A wait that the abort then ends writes
//   its status (3) into the page-locked block only: the shared status word never shows it.  The host
//   reads the shared abort word before the status (`LoopbackComm.failed`), so it reports the failure all
//   the same; only a timed-out wait (2) reaches the shared status word.
// * The thread makes no HIP call, only loads and stores, but it must not poll the page-locked block
//   while the HIP runtime unmaps it at process exit: the owner calls stop() before that
//   (parallel/loopback_comm.py does, from an exit hook, for every relay no abort has ended).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

namespace adapt {

class LbRelay {
 public:
  // `shared`: the mapped control block of `bytes`; word offsets are in bytes, 8-aligned, each one u64.
  // `abort_word` is the `in` word that ends every wait: once it is mirrored non-zero the relay's work is
  // over and its thread ends.  Allocates on the calling thread's current device; throws on a HIP error.
  LbRelay(void* shared, size_t bytes, std::vector<size_t> out_words, std::vector<size_t> in_words,
          size_t abort_word);
  // stop() and raise the abort word in the page-locked block, so a wait still pending there ends.  The
  // block itself is never freed: kernels already enqueued may still read it.
  ~LbRelay();
  void stop();                                     // end the thread (idempotent); nothing is mirrored after
  LbRelay(const LbRelay&) = delete;
  LbRelay& operator=(const LbRelay&) = delete;

  uintptr_t dev() const { return reinterpret_cast<uintptr_t>(dev_); }   // the block's device address

 private:
  void run();
  bool mirror();                                   // one pass; true once the abort word has been mirrored

  unsigned char* shared_;
  unsigned char* pinned_ = nullptr;
  void* dev_ = nullptr;
  std::vector<size_t> out_, in_;
  size_t abort_;
  std::atomic<bool> stop_{false};
  std::thread thread_;
};

}  // namespace adapt
