// Device side of the certificate of high-order hexahedra (tm_highorder3_cert.hip, K17): what it borrows from K11 and K16.
#pragma once
#include "tm_highorder3_cert.hpp"
#include "tm_highorder3_dev.hpp"
#include "tm_highorder_cert_dev.hpp"

namespace tmh {

// span elements per window of fine planes for a block of ni x nj nodes with Eg span elements (the plane budget, or its override)
uint64_t h3_window_elements(int order, uint64_t ni, uint64_t nj, uint64_t Eg);

}  // namespace tmh
