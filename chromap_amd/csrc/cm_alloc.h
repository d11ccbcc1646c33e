// cm_alloc.h -- the serial piece of --allocate-multi-mappings (MappingProcessor::AllocateMultiMappings, mapping_processor.h:319-440):
// one std::mt19937 for the whole run, one std::discrete_distribution<uint32_t> per read whose weights do not sum to 0, reads visited in
// ascending read_id.  How much of the generator a read consumes is the library's business (a one-member group draws nothing in
// libstdc++), so the classes themselves are used, in a loop shaped like the reference's (:384-431).  Host code only: the device
// stage of cm_post.hip downloads the weights and uploads the kept positions; the host writers of cm_host.cpp call it directly.
#ifndef CM_ALLOC_H_
#define CM_ALLOC_H_
#include <stdint.h>

#include <random>
#include <vector>

#define CM_ALLOC_MIN_UNIQUE_MAPQ 4     // min_unique_mapping_mapq_ (chromap.h:199): a surviving record below it is a multi-mapping
#define CM_ALLOC_HEAD 0x80000000u      // set in the weight of a read's first member

// [interval_start, interval_end) of a multi-mapping's neighbourhood (mapping_processor.h:270-275), in the reference's own 32-bit arithmetic
static inline void cm_alloc_interval(uint32_t start, uint32_t end, int32_t distance, uint32_t *qs, uint32_t *qe) {
  *qs = start > (uint32_t)distance ? start - (uint32_t)distance : 0;
  *qe = end + (uint32_t)distance;
}

// w[0 .. m): the multi-mappings' weights in (read_id, sorted position) order, CM_ALLOC_HEAD set where a read begins.  kept: for every
// read whose weights sum to more than 0, the index of the member it is given to.  Returns the reads whose weights sum to 0
static inline uint64_t cm_alloc_draw(const uint32_t *w, uint64_t m, int32_t seed, std::vector<uint32_t> &kept) {
  std::mt19937 generator(seed);
  std::vector<uint32_t> weights;
  uint64_t without_overlap = 0;
  kept.clear();
  for (uint64_t first = 0; first < m;) {
    uint64_t end = first + 1;
    while (end < m && !(w[end] & CM_ALLOC_HEAD)) ++end;
    weights.clear();
    uint32_t sum_weight = 0;  // (32 bits, as the reference's)
    for (uint64_t i = first; i < end; ++i) { weights.emplace_back(w[i] & ~CM_ALLOC_HEAD); sum_weight += weights.back(); }
    if (sum_weight == 0) {
      ++without_overlap;
    } else {
      std::discrete_distribution<uint32_t> distribution(weights.begin(), weights.end());
      kept.push_back((uint32_t)(first + distribution(generator)));
    }
    first = end;
  }
  return without_overlap;
}

// The whole stage on the host, for the writers of cm_host.cpp: survivors of duplicate removal in output order, each
// (rid, start, end, mapq, read_id) after the in-memory Tn5 shift.  keep[i] = 0 for the multi-mappings that go nowhere
struct CmAllocRec { uint32_t rid, start, end, mapq, read_id; };
struct CmAllocCounts { uint64_t n_multi = 0, n_allocated = 0, n_without_overlap = 0; };
CmAllocCounts cm_alloc_host(const std::vector<CmAllocRec> &recs, int32_t distance, int32_t seed, std::vector<uint8_t> &keep);
#endif
