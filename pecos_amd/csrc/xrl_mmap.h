// Reader of the reference's memory-mapped container (*.mmap_store; layout in xrl_mmap.cpp), shared by the model loader and the HNSW loader.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "xrl_common.h"

namespace xrl {

class MmapReader {
public:
    explicit MmapReader(const std::string& path) : path_(path) {
        fd_ = ::open(path.c_str(), O_RDONLY);
        if (fd_ < 0) fail("cannot open " + path);
        struct stat st;
        if (::fstat(fd_, &st) != 0 || st.st_size < 24) { ::close(fd_); fail(path + " is not a valid PECOS MMAP file."); }
        n_ = (size_t)st.st_size;
        void* m = ::mmap(nullptr, n_, PROT_READ, MAP_PRIVATE, fd_, 0);
        if (m == MAP_FAILED) { ::close(fd_); fail("cannot mmap " + path); }
        p_ = (const uint8_t*)m;
        const uint8_t magic[6] = {0x93u, 'P', 'E', 'C', 'O', 'S'};
        const uint8_t* sig = p_ + n_ - 16;
        if (std::memcmp(sig, magic, 6) != 0) fail(path + ": File is not a valid PECOS MMAP file.");
        if (sig[6] != (uint8_t)'<') fail(path + ": Inconsistent endianness between runtime and the mmap file.");
        if (sig[7] != 1) fail(path + ": Inconsistent version between code and the mmap file.");
        uint64_t meta; std::memcpy(&meta, sig + 8, 8);
        if (meta + 8 > n_) fail(path + ": corrupt mmap metadata");
        uint64_t nb; std::memcpy(&nb, p_ + meta, 8);
        if (meta + 8 + nb * 16 > n_) fail(path + ": corrupt mmap metadata");
        blocks_.resize(nb);
        for (uint64_t i = 0; i < nb; ++i) {
            std::memcpy(&blocks_[i].first, p_ + meta + 8 + i * 16, 8);
            std::memcpy(&blocks_[i].second, p_ + meta + 16 + i * 16, 8);
            if (blocks_[i].first + blocks_[i].second > meta) fail(path + ": mmap block out of range");
        }
    }
    MmapReader(const MmapReader&) = delete;
    MmapReader& operator=(const MmapReader&) = delete;
    ~MmapReader() { if (p_) ::munmap((void*)p_, n_); if (fd_ >= 0) ::close(fd_); }
    template <class T> T one() { const T* p = many<T>(1); return *p; }
    template <class T> const T* many(uint64_t count) {
        if (it_ >= blocks_.size()) fail(path_ + ": mmap file has fewer blocks than expected");
        const auto b = blocks_[it_++];
        if (b.second != count * sizeof(T)) fail(path_ + ": unexpected mmap block size");
        return reinterpret_cast<const T*>(p_ + b.first);
    }
    template <class T> const T* vec(uint64_t& size) { size = one<uint64_t>(); return many<T>(size); }
private:
    std::string path_; int fd_ = -1; const uint8_t* p_ = nullptr; size_t n_ = 0;
    std::vector<std::pair<uint64_t, uint64_t>> blocks_; size_t it_ = 0;
};

}  // namespace xrl
