// The C++ host's sgd_step writes the next step's filter packs (unet_sgd_step_packed) and the next loss_and_backward claims them
// (UNET_MODE_PACKS_CURRENT): the sequence must equal the unfused one (pack_in_update = false) bit for bit, also when the parameters
// are touched between the update and the next forward (torch in-place op, copy_from), which must make that forward repack.
// Exit code 0 and "OK" on success.
#include "unet.hpp"
#include <iostream>

#define REQUIRE(cond, msg) do { if (!(cond)) { std::cerr << "FAILED: " << msg << std::endl; return 1; } } while (0)

int main() {
    if (!torch::cuda::is_available()) { std::cerr << "needs a GPU" << std::endl; return 2; }
    torch::manual_seed(0);
    const std::string arch = "conv16,ks3,stride1+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu\n"
                             "conv32,ks3,stride2+norm,leaky_relu+conv32,ks3,stride1+norm,leaky_relu+conv_trans16,ks2,stride2\n"
                             "conv16,ks3,stride1+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv4,ks1,stride1";
    torch::Device dev(torch::kCUDA, 0);
    UNet3d a(1, 4, arch), b(1, 4, arch), c(1, 4, arch);
    a->to(dev); b->to(dev); c->to(dev);
    b->copy_from(*a); c->copy_from(*a);
    a->train(); b->train(); c->train();
    REQUIRE(a->pack_in_update, "the fused update is the default");
    b->pack_in_update = false;
    auto x = torch::rand({1, 1, 32, 32, 32}, torch::TensorOptions().device(dev));
    auto x2 = torch::rand({1, 1, 16, 16, 16}, torch::TensorOptions().device(dev));
    auto tgt = torch::randint(0, 4, {1, 32, 32, 32}, torch::TensorOptions().dtype(torch::kLong).device(dev));
    auto tgt2 = torch::randint(0, 4, {1, 16, 16, 16}, torch::TensorOptions().dtype(torch::kLong).device(dev));
    for (int stp = 0; stp < 6; ++stp) {
        const bool small = stp == 4;                       // another size in between: its workspace has no packs yet
        auto la = a->loss_and_backward(small ? x2 : x, small ? tgt2 : tgt, true, true, true);
        auto lb = b->loss_and_backward(small ? x2 : x, small ? tgt2 : tgt, true, true, true);
        REQUIRE(torch::equal(la, lb), "losses of step " + std::to_string(stp));
        a->sgd_step(0.01f, 1.0f);
        b->sgd_step(0.01f, 1.0f);
        torch::NoGradGuard ng;
        if (stp == 1) {                                    // an in-place torch op on one parameter behind the update
            a->parameters()[2].mul_(1.5f);
            b->parameters()[2].mul_(1.5f);
        }
        if (stp == 2) { a->copy_from(*c); b->copy_from(*c); }   // train.cpp:573-579
        REQUIRE(torch::equal(a->flat_params, b->flat_params), "parameters after step " + std::to_string(stp));
    }
    torch::cuda::synchronize();
    REQUIRE(torch::equal(a->flat_params, b->flat_params), "parameters");
    REQUIRE(torch::equal(a->flat_grads, b->flat_grads) && a->flat_grads.abs().max().item<float>() == 0.f, "gradients are cleared");
    std::cout << "OK sgd_pack_host" << std::endl;
    return 0;
}
