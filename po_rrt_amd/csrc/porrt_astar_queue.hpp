// porrt_astar_queue.hpp -- the open list of the TAMP-RRT A* search (porrt_tamp_astar.hpp): a binary min-heap of
// (priority, id) pairs.  Plain C++, no HIP: tests/astar_queue_check.cpp builds it on its own under the sanitizers.
//
// The order is OURS, not the reference's.  The reference's Priority::cmp (common.rs:235-239) never says Equal, so which of two
// equal priorities its PriorityQueue pops first is a property of that crate's heap layout, not of the algorithm.  Here:
//   - the lower priority pops first (compared as doubles, so +0.0 and -0.0 are equal, and +inf sorts after every finite value);
//   - equal priorities pop in ASCENDING ID.
// That is a strict total order on the entries of one search (ids are unique), so the pop sequence is a function of the set of
// pushed entries alone, never of the order of the pushes or of the heap's shape.  NaN priorities are the caller's to refuse:
// they compare false both ways and would fall back to the id order.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace porrt_astar {

struct QueueEntry {
    double priority;
    uint64_t id;
};

// a before b in pop order
static inline bool queue_before(const QueueEntry &a, const QueueEntry &b) {
    if (a.priority < b.priority) return true;
    if (b.priority < a.priority) return false;
    return a.id < b.id;
}

class Queue {
public:
    bool empty() const { return h_.empty(); }
    size_t size() const { return h_.size(); }
    const QueueEntry &top() const { return h_.front(); }
    void clear() { h_.clear(); }
    void push(double priority, uint64_t id) {
        h_.push_back({priority, id});
        size_t i = h_.size() - 1;
        while (i > 0) {
            const size_t p = (i - 1) / 2;
            if (!queue_before(h_[i], h_[p])) break;
            std::swap(h_[i], h_[p]);
            i = p;
        }
    }
    QueueEntry pop() {
        const QueueEntry out = h_.front();
        h_.front() = h_.back();
        h_.pop_back();
        const size_t n = h_.size();
        size_t i = 0;
        while (true) {
            const size_t l = 2 * i + 1, r = l + 1;
            size_t m = i;
            if (l < n && queue_before(h_[l], h_[m])) m = l;
            if (r < n && queue_before(h_[r], h_[m])) m = r;
            if (m == i) break;
            std::swap(h_[i], h_[m]);
            i = m;
        }
        return out;
    }

private:
    std::vector<QueueEntry> h_;
};

} // namespace porrt_astar
